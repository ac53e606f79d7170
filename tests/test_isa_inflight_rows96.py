"""tests/test_isa_inflight.py's check on the 96-row form of the k = 7 split kernel (conv1d_bsplit96.hip, its own translation unit):
the named landing registers of csrc/inflight_regs.h are touched by nothing between the load that writes them and the v_cndmask that
takes the value out, and the kernel -- 96 accumulators and two fragment sets per MFMA wave -- spills no vector register."""
import os
import shutil
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_rows96_kernel_keeps_its_landing_registers_and_does_not_spill():
    import check_inflight_regs as C
    asm = C.compile_to_asm(os.path.join(REPO, "facodec_amd", "csrc", "conv1d_bsplit96.hip"))
    res = C.reserved_violations(asm)
    assert len(res) == 1, sorted(res)
    assert [lo for lo, _ in res.values()] == [208]
    live = C.named_lifetime_violations(asm)
    assert set(live) == set(res)
    for name, bad in live.items():
        assert not bad, (name, bad[:5])
    spills = C.spill_counts(asm)
    assert spills and max(spills.values()) == 0, spills
