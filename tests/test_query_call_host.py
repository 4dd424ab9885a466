"""CPU: the parts of pintron_amd/csrc/pgpu_query_call.h that make no HIP call (the rounding of the device offsets, the
return code of a HIP error, the range checks of the refine and chain queries, the validator and the device layout the two
chained entries share), in a stand-alone program
(tests/hostcheck/query_call_check.cpp) built by the host compiler with AddressSanitizer and UBSan and run directly."""
import os
import subprocess

import pytest

import resource_lib

HERE = os.path.dirname(os.path.abspath(__file__))


def test_host_parts_of_the_query_header_under_sanitizers(tmp_path):
    hipcc = resource_lib.hipcc()
    if not hipcc:
        pytest.skip("no ROCm headers here")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / "query_call_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + include, "-o", exe,
                    os.path.join(HERE, "hostcheck", "query_call_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout, r.stderr[-2000:])
