"""What the compiler made of pgpu_refine.hip (no GPU needed: hipcc cross-compiles gfx950 here): the checks of
test_kernel_resources.py for the intron-border kernel -- no scratch, no spilled vector registers."""
from resource_lib import usage as _usage


def test_refine_kernel_has_no_stack_frame(tmp_path):
    usage = _usage("pgpu_refine.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "refine_kernel" in k}
    assert len(kernels) == 1, sorted(usage)
    for name, u in kernels.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] <= 8192, (name, u)             # rows, two operands, three diagonals
