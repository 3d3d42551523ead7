"""CPU-side audit (no GPU needed) of the prologues of the loss op's two patch kernels in the built gfx950 code of libwarprnnt.so,
in the way of tests/test_isa_audit.py: a patch workgroup holds 26.9 KB of LDS for its whole life, so every serial wait in that life
that is not the logits stream costs bytes in flight.

  lsm pass       cell_tile_kernel<32, false, true, true>: the cell's label is fetched BEFORE the logits are staged -- no plain global
                 load between the staging barrier and the edge-store barrier; the decay statistic is summed by one wave on DPP row
                 operations + v_readlane -- no ds_bpermute anywhere in the kernel.
  gradient pass  cell_tile_kernel<32, true, true, true>: lin_grad_setup asks for everything a cell needs in ONE batch of vector
                 loads -- in front of the first barrier, no global load follows the first vector-memory wait."""
import os
import re

import pytest

from tests.test_isa_audit import OBJDUMP, READELF, _find, kernels  # noqa: F401  (kernels: that module's fixture, the disassembly)

pytestmark = pytest.mark.skipif(not (os.path.exists(READELF) and os.path.exists(OBJDUMP)), reason="ROCm LLVM tools absent")

LSM = "Li32ELb0ELb1ELb1ELb0E"   # <VP = 32, GRAD = false, AL = true, LIN = true, FE = false>
GRAD = "Li32ELb1ELb1ELb1ELb0E"  # <VP = 32, GRAD = true, AL = true, LIN = true, FE = false>


def _plain_loads(text):
    """global_load_dword[xN] instructions that are not the LDS-DMA forms (global_load_lds_dword...)."""
    return re.findall(r"\bglobal_load_dword\w*", text)  # (the LDS-DMA mnemonics read global_load_lds_...: no match)


def _kernel(asm, needle):
    hits = _find(asm, "cell_tile_kernel", needle)
    assert len(hits) == 1, hits
    return asm[hits[0]]


def test_the_matcher_tells_plain_loads_from_lds_dma():
    probe = "global_load_lds_dwordx4 v[1:2], off\nglobal_load_dword v3, v[4:5], off\nglobal_load_dwordx2 v[6:7], v8, s[0:1]\n"
    assert _plain_loads(probe) == ["global_load_dword", "global_load_dwordx2"]


def test_lsm_fetches_nothing_between_its_barriers_and_reduces_in_registers(kernels):
    _, asm = kernels
    k = _kernel(asm, LSM)
    parts = re.split(r"\bs_barrier\b", k)
    assert len(parts) == 3, len(parts)  # two barriers: logits staged; edge probabilities in the cells' slots
    assert "global_load_lds_dwordx4" in parts[0]  # the staging loop is where it is expected
    assert _plain_loads(parts[1]) == [], _plain_loads(parts[1])
    assert "ds_bpermute" not in k
    assert "v_readlane_b32" in parts[1] and len(re.findall(r"v_add_f32_dpp", parts[1])) >= 4  # the statistic's row sums
    assert _plain_loads(parts[0]), "the label is fetched in front of the staging barrier"


def test_gradient_setup_is_one_vector_batch(kernels):
    _, asm = kernels
    k = _kernel(asm, GRAD)
    head = re.split(r"\bs_barrier\b", k)[0]
    assert len(_plain_loads(head)) >= 9, _plain_loads(head)  # A, Bt x 3, EA, EB x 3, the label
    first_wait = re.search(r"s_waitcnt[^\n]*vmcnt\(", head)
    assert first_wait, "no vector-memory wait in front of the first barrier"
    after = head[first_wait.start():]
    assert _plain_loads(after) == [], _plain_loads(after)


def test_patch_kernels_keep_their_register_budget(kernels):
    meta, _ = kernels
    for needle in (LSM, GRAD):
        for name in _find(meta, "cell_tile_kernel", needle):
            assert int(meta[name]["vgpr_count"]) <= 80 and int(meta[name]["private_segment_fixed_size"]) == 0, (name, meta[name])
