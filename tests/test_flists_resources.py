"""What the compiler made of pgpu_flists.hip (no GPU needed: hipcc cross-compiles gfx950 here): the one-wave-per-EST selection
kernel without scratch and without a spilled vector register, with the 1 024 bytes of LDS the file's head comment states (the
exons of to_add; the list is a mask in scalar registers), and the thread-per-candidate and thread-per-EST hand-off kernels
without a stack frame or LDS.  The compiler reports 42 vector registers for the selection kernel; the bound below leaves
some twenty more before the test asks why."""
from resource_lib import usage as _usage

HANDOFFS = ("flist_owner_kernel", "flist_to_clean_kernel", "flist_clean_to_select_kernel", "flist_select_to_gaps_kernel",
            "flist_gaps_verdict_kernel", "flist_gaps_to_refine_kernel", "flist_gather_kernelILb0", "flist_gather_kernelILb1")


def test_flists_kernels_have_no_stack_frame_and_the_stated_lds(tmp_path):
    usage = _usage("pgpu_flists.hip", tmp_path)
    assert len(usage) == 9, sorted(usage)
    select = [u for name, u in usage.items() if "flist_select_kernel" in name]
    assert len(select) == 1
    assert select[0]["ScratchSize"] == 0 and select[0]["VGPRs Spill"] == 0 and select[0]["SGPRs Spill"] == 0, select
    assert select[0]["LDS Size"] == 1024, select
    assert select[0]["VGPRs"] <= 64, select
    for part in HANDOFFS:
        found = [u for name, u in usage.items() if part in name]
        assert len(found) == 1, part
        assert found[0]["ScratchSize"] == 0 and found[0]["VGPRs Spill"] == 0 and found[0]["LDS Size"] == 0, (part, found)
