"""What the compiler made of pgpu_unit.hip (no GPU needed: hipcc cross-compiles gfx950 here): the two instances of
unit_kernel -- the count pass and the write pass -- run one thread per unit over records of 16 to 32 bytes and the exons
behind an index: no scratch, no spilled register, no LDS.  The file holds no other kernel: the scan is launched from its
own file."""
from resource_lib import usage as _usage


def test_the_unit_kernels_have_no_scratch_no_spill_and_no_lds(tmp_path):
    usage = _usage("pgpu_unit.hip", tmp_path)
    assert all("unit_kernel" in k for k in usage) and len(usage) == 2, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] == 0, (name, u)
