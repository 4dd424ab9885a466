"""What the compiler made of pgpu_chain.hip (no GPU needed: hipcc cross-compiles gfx950 here): the checks of
test_refine_resources.py for the kernel that chains the introns of a factorization -- no scratch, no spilled vector
registers, and the LDS of one wave: the traceback's direction window and path, with the decision's buffers laid over
them (the direction bytes themselves live in HBM: DESIGN.md section 5e)."""
from resource_lib import usage as _usage


def test_chain_kernel_has_no_stack_frame(tmp_path):
    usage = _usage("pgpu_chain.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "chain_kernel" in k}
    assert len(kernels) == 1, sorted(usage)
    for name, u in kernels.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] <= 8192 + 704, (name, u)       # TB_WIN_BYTES + TB_PATH; RefineLds (5.6 KB) shares them
