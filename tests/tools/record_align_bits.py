"""Records tests/golden/align/align_bits.npz, the fixture of tests/test_align_bits_gpu.py, on an MI355X: the SHA-256 of every
input, the outputs of every case of tests/align_bits_cases.py and the three workspace sizes at the cases' shapes.

    python tests/tools/record_align_bits.py [--package-root DIR] [--out FILE]

The fixture pins what a build computed, so it is recorded from the build one wants pinned: --package-root names a checkout (built)
of that commit, whose package is imported in place of this tree's; the case list is this tree's either way."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import align_bits_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", cases.FIXTURE))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch

    import rnnt_speech_recognition_amd as pkg

    assert os.path.abspath(pkg.__file__).startswith(os.path.abspath(a.package_root) + os.sep), pkg.__file__
    assert torch.cuda.is_available(), "the fixture is recorded on the GPU"
    pkg.build()
    dev = torch.device("cuda:0")
    rec = {}
    for index, case in enumerate(cases.CASES):
        inp = cases.inputs(case, index)
        for name, x in zip(cases.INPUT_NAMES, inp):
            rec[f"{case['name']}/sha256/{name}"] = np.array(cases.sha256(x))
        for k, o in enumerate(cases.run(case, inp, dev)):
            rec[f"{case['name']}/out{k}"] = o
        print(case["name"], "scores", rec[f"{case['name']}/out{2 if case['topology'] != 'tdt' else 3}"], flush=True)
    rec["workspace/shapes"] = np.array(cases.workspace_names())
    rec["workspace/bytes"] = np.array([cases.workspace_bytes(*s) for s in cases.workspace_shapes()], dtype=np.int64)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes,", len(cases.CASES), "cases from", pkg.__file__)


if __name__ == "__main__":
    main()
