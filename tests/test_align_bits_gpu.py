"""The three forced aligners give the bits they gave before their kernel files shared csrc/rnnt_align_parts.h: every output of
every case of tests/align_bits_cases.py, byte for byte, against tests/golden/align/align_bits.npz -- recorded by
tests/tools/record_align_bits.py from a build of the commit BEFORE the sharing.  The bits depend on the chunk-to-lane map and the
merge order of the cell pass and on the strict-greater tie rule of the sweeps; the cases reach every lanes-per-cell width, both load
routes, every loader of the path kernels, the 1024-thread kernel, the TDT chunk that straddles the token / duration boundary and the
slab route.  The inputs' SHA-256 is asserted first: a generator that drifted reads as a fixture problem, not as a kernel bug.

The workspace sizes are host code and are compared here as well, without a device."""
import os

import numpy as np
import pytest

import rnnt_speech_recognition_amd as pkg
from tests import align_bits_cases as cases


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, cases.FIXTURE))


def test_workspace_sizes_are_the_recorded_ones(golden):
    pkg.build()
    assert cases.workspace_names() == golden["workspace/shapes"].tolist()
    assert [cases.workspace_bytes(*s) for s in cases.workspace_shapes()] == golden["workspace/bytes"].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(cases.CASES)), ids=[c["name"] for c in cases.CASES])
def test_outputs_are_bitwise_the_recorded_ones(golden, index):
    import torch

    assert torch.cuda.is_available()
    pkg.build()
    case = cases.CASES[index]
    inp = cases.inputs(case, index)
    for name, x in zip(cases.INPUT_NAMES, inp):
        assert cases.sha256(x) == str(golden[f"{case['name']}/sha256/{name}"]), f"the fixture was recorded on other inputs: {name}"
    out = cases.run(case, inp, torch.device("cuda:0"))
    assert len(out) == (4 if case["topology"] == "tdt" else 3)
    for k, got in enumerate(out):
        want = golden[f"{case['name']}/out{k}"]
        assert got.dtype == want.dtype and got.shape == want.shape, (k, got.dtype, got.shape)
        assert got.tobytes() == want.tobytes(), (case["name"], k)
