"""What the compiler made of pgpu_chain.hip (no GPU needed: hipcc cross-compiles gfx950 here): the checks of
test_refine_resources.py for the kernel that chains the introns of a factorization -- no scratch, no spilled vector
registers, and the LDS of one wave: the traceback's direction window and path, with the decision's buffers laid over
them (the direction bytes themselves live in HBM: DESIGN.md section 5e)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pintron_amd", "csrc")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def test_chain_kernel_has_no_stack_frame(tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc here")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "pgpu_chain.hip", "-o",
                        str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"],
                       cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    kernels = {k: v for k, v in usage.items() if "chain_kernel" in k}
    assert len(kernels) == 1, sorted(usage)
    for name, u in kernels.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] <= 8192 + 704, (name, u)       # TB_WIN_BYTES + TB_PATH; RefineLds (5.6 KB) shares them
