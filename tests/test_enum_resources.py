"""What the compiler made of pgpu_enum.hip (no GPU needed: hipcc cross-compiles gfx950 here): the two instances of the
one-wave-per-record kernel, the count pass and the write pass, and nothing else; no scratch -- the walk's stack, the lists
and the pool of embeddings are in LDS, its counters and masks in registers -- no spilled vector registers, and the 19 588
bytes of LDS the file's head comment states (struct State).  The compiler reports 48 and 51 vector registers; the bound
below leaves a dozen more before the test asks why."""
from resource_lib import usage as _usage


def test_enum_kernels_have_no_stack_frame_and_the_stated_lds(tmp_path):
    usage = _usage("pgpu_enum.hip", tmp_path)
    assert len(usage) == 2 and all("enum_kernel" in name for name in usage), sorted(usage)
    assert {name[name.index("enum_kernelILb") + len("enum_kernelILb")] for name in usage} == {"0", "1"}, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] == 19588, (name, u)
        assert u["VGPRs"] <= 64, (name, u)
