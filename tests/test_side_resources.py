"""What the compiler made of pgpu_side.hip (no GPU needed: hipcc cross-compiles gfx950 here): the count pass -- one thread
per unit -- and the write pass -- one wave per unit, whose copy loop keeps nothing per thread: no scratch, no spilled
register, and the LDS the file's head comment states.  The file holds no other kernel: the scans are launched from their own
file."""
import os
import re

from resource_lib import CSRC, usage as _usage


def test_the_side_kernels_have_no_scratch_no_spill_and_the_stated_lds(tmp_path):
    head = open(os.path.join(CSRC, "pgpu_side.hip")).read().split("#include", 1)[0]
    stated = re.search(r"^// LDS: (\d+) bytes", head, re.M)
    assert stated, "the head comment of pgpu_side.hip states its LDS"
    usage = _usage("pgpu_side.hip", tmp_path)
    assert sorted(k for k in usage if "side_count_kernel" in k or "side_write_kernel" in k) == sorted(usage) and len(usage) == 2, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] == int(stated.group(1)), (name, u)
