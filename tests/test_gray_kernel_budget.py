"""The co-residency budget of the gray kernels (MI355_F_GRAY), read from the code objects the way
test_kernel_budget.py reads the RGB ones: batched gray calls run a part's tail kernels under the next part's block
encode, so two k_gray_encode workgroups plus two of the half-window k_gray_merge (one of the full-window form) must fit
a CU -- at most 512 registers per SIMD lane, 160 KiB of LDS -- with no scratch, and the per-frame k_gray_dc_heads stays
as light as k_dc_heads."""
import os

import pytest

import test_kernel_budget as kb

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(kb.LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")


def test_gray_kernels_fit_beside_the_gray_block_encode(tmp_path):
    assert os.path.exists(kb.LIB), "libmi355jpeg.so not built"
    t = kb.kernel_table(tmp_path)
    enc = {k: v for k, v in t.items() if "k_gray_encodeILb0E" in k}  # the shipped (non-probe) form
    merge = {k: v for k, v in t.items() if "k_gray_mergeIL" in k}    # <SMALL>: full window (one per CU), half (two)
    assert len(enc) == 1 and len(merge) == 2, sorted(t)
    for k, v in {**enc, **{k: v for k, v in t.items() if "k_gray_" in k}}.items():
        assert v["scratch"] == 0, (k, v)
    e = next(iter(enc.values()))
    for mk, m in merge.items():
        per_cu = 2 if "ILb1EE" in mk else 1
        lds = 2 * kb.up(e["lds"], 1280) + per_cu * kb.up(m["lds"], 1280)
        regs = 2 * kb.up(e["vgpr"], 8) + per_cu * kb.up(m["vgpr"], 8)
        assert m["vgpr"] <= kb.up(m["used"], 8), (mk, m)  # no occupancy-driven inflation of the allocation
        assert lds <= 160 * 1024, (mk, e, m, lds)
        assert regs <= 512, (mk, e, m, regs)
    heads = [v for k, v in t.items() if "k_gray_dc_heads" in k]
    assert len(heads) == 1 and heads[0]["vgpr"] <= 32 and heads[0]["lds"] <= 1280
