"""What the compiler made of the hot kernels (no GPU needed: hipcc cross-compiles gfx950 here).

Round 4 found `dp_batch_kernel` writing three times its bytes to HBM because ONE device routine had been left as a
call: the call gave the kernel a stack frame (96 B of scratch per lane) and every wave paid for it, whether the
routine ran or not.  Nothing in the parity tests can see that, and the profile that did was
taken by chance -- so the resource usage the compiler reports is pinned here: no scratch, no spilled vector
registers, at most 128 VGPRs (four waves per SIMD), and the LDS budget that lets four workgroups share a CU."""
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


def _usage(source, tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc here")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", source, "-o",
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


def test_dp_kernels_have_no_stack_frame(tmp_path):
    usage = _usage("pgpu_dp_kernels.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "kernel" in k}
    assert any("dp_batch_kernel" in k for k in kernels), sorted(usage)[:5]
    for name, u in kernels.items():
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u.get("VGPRs Spill", 0) == 0, (name, u)
    batch = [u for k, u in kernels.items() if "dp_batch_kernel" in k][0]
    assert batch["VGPRs"] <= 128 and batch["Occupancy"] >= 4, batch
    # the dynamic LDS is bounded by WAVE_JOBS_LDS's static_assert, which allows for 256 B of static LDS
    assert batch["LDS Size"] <= 256, batch
