"""What the compiler made of the hot kernels (no GPU needed: hipcc cross-compiles gfx950 here).

Round 4 found `dp_batch_kernel` writing three times its bytes to HBM because ONE device routine had been left as a
call: the call gave the kernel a stack frame (96 B of scratch per lane) and every wave paid for it, whether the
routine ran or not.  Nothing in the parity tests can see that, and the profile that did was
taken by chance -- so the resource usage the compiler reports is pinned here: no scratch, no spilled vector
registers, at most 128 VGPRs (four waves per SIMD), and the LDS budget that lets four workgroups share a CU."""
from resource_lib import usage as _usage


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
