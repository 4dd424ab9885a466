"""The ctypes structs and numpy dtypes of pintron_amd/capi.py held against the typedefs of include/pintron_gpu.h."""
import ctypes as C
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pintron_gpu.h")
SIZE_OF = {"uint64_t": 8, "uint32_t": 4, "int32_t": 4, "double": 8}


def header_struct(name):
    """`typedef struct { ... } name;  /* N bytes` of the header -> ([(field, C type)], N)"""
    text = open(HEADER).read()
    m = re.search(r"typedef struct \{((?:(?!typedef).)*?)\}\s*" + name + r";\s*/\*\s*(\d+) bytes", text, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields, int(m.group(2))


def assert_layout(cname, struct, dtype):
    """the header's struct `cname`, the ctypes `struct` and the numpy `dtype` have the same fields in the same order, at the
    same offsets, of the same sizes, and the size the header's comment states"""
    fields, size = header_struct(cname)
    assert [f for f, _ in fields] == [f for f, _ in struct._fields_] == [f for f, _ in dtype], cname
    off = 0
    dt = np.dtype(dtype)
    for f, ctype in fields:                          # no padding anywhere: every field follows the one before
        assert getattr(struct, f).offset == off == dt.fields[f][1], (cname, f)
        assert getattr(struct, f).size == SIZE_OF[ctype] == dt.fields[f][0].itemsize, (cname, f)
        off += SIZE_OF[ctype]
    assert off == size == C.sizeof(struct) == dt.itemsize, cname
