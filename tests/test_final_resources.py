"""What the compiler made of pgpu_final.hip (no GPU needed: hipcc cross-compiles gfx950 here): the three hand-off kernels
of the final driver -- final_to_tail_kernel, final_tail_to_small_kernel and the two instances of final_gather_kernel -- run
one thread per EST over records of 16 to 32 bytes and a handful of exons behind an index: no scratch, no spilled register,
no LDS.  The file holds no other kernel: the two stage kernels are launched from their own files."""
from resource_lib import usage as _usage


def test_the_hand_off_kernels_have_no_scratch_no_spill_and_no_lds(tmp_path):
    usage = _usage("pgpu_final.hip", tmp_path)
    names = ("final_to_tail_kernel", "final_tail_to_small_kernel", "final_gather_kernel")
    assert all(any(n in k for n in names) for k in usage), sorted(usage)
    for n, count in zip(names, (1, 1, 2)):
        assert sum(n in k for k in usage) == count, (n, sorted(usage))
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] == 0, (name, u)
