"""CPU: the exact-occurrence query (pgpu_index_find) is exported, bound and documented in the header, has no CPU
fallback, and its kernels use no scratch memory and spill no register (hipcc cross-compiles gfx950 here)."""
import ctypes as C
import os
import re

import pytest

from resource_lib import usage as _usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    import pintron_amd.capi as capi
    return capi


def test_find_is_exported_and_bound(capi):
    L = capi.lib()
    assert hasattr(L, "pgpu_index_find") and hasattr(L, "pgpu_index_find_kernel_ms")
    assert "pgpu_index_find" in capi.EXPORTS
    assert C.sizeof(capi.FindQuery) == 24
    assert [f[0] for f in capi.FindQuery._fields_] == ["pat_off", "pat_len", "reserved", "lo", "hi"]
    assert capi.FindQuery.lo.offset == 16 and capi.FindQuery.hi.offset == 20
    hdr = open(os.path.join(ROOT, "include", "pintron_gpu.h")).read()
    assert re.search(r"\bint\s+pgpu_index_find\s*\(", hdr) and "pgpu_find_query" in hdr
    assert L.pgpu_abi_version() == 1                      # the change is additive
    assert hasattr(capi.Index, "find")
    assert L.pgpu_index_find_kernel_ms(0) == 0.0


def test_find_rejects_bad_arguments_without_a_device(capi):
    L = capi.lib()
    first = (C.c_uint64 * 2)()
    n_out = C.c_size_t(7)
    q = (capi.FindQuery * 1)(capi.FindQuery(0, 3, 0, 0, 10))
    assert L.pgpu_index_find(None, None, b"ACG", 3, q, 1, None, 0, first, C.byref(n_out)) == capi.PGPU_EINVAL


def test_find_has_no_cpu_fallback(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(capi.PgpuError) as e:
        capi.Context(0)                                   # no context, no index, no query
    assert e.value.code == capi.PGPU_EDEVICE


def test_find_kernels_have_no_stack_frame(tmp_path):
    usage = _usage("pgpu_find.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "kernel" in k}
    assert any("find_count_kernel" in k for k in kernels) and any("find_fill_kernel" in k for k in kernels), sorted(usage)
    for name, u in kernels.items():
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
    fill = [u for k, u in kernels.items() if "find_fill_kernel" in k][0]
    assert fill["LDS Size"] <= 16 * 1024, fill            # the sort buffer of one wave: ten workgroups share a CU
