"""What the compiler reports for the kernels of one HIP source (no GPU needed: hipcc cross-compiles gfx950): the
`-Rpass-analysis=kernel-resource-usage` remarks as a dict per function.  Shared by the resource tests
(test_kernel_resources.py, test_find_cpu.py, test_classify_cpu.py, test_refine_resources.py, test_chain_resources.py)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pintron_amd", "csrc")


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def usage(source, tmp_path):
    """{function name: {remark: number}} for pintron_amd/csrc/<source>; skips where there is no hipcc"""
    cc = hipcc()
    if not cc:
        pytest.skip("no hipcc here")
    r = subprocess.run([cc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", source, "-o",
                        str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"],
                       cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out
