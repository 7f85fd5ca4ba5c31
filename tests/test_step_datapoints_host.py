"""mgn_step_datapoints without a GPU: the symbol is declared, exported and bound with the header's signature on the ctypes and the
Julia side (through tests/test_julia_shim.py's parsers), the ABI version stands, and the Python classes offer what they should."""
import ctypes as C
import os
import re

import test_julia_shim as js
from mgn_amd import Engine, _capi

SYM = "mgn_step_datapoints"
# (mgn_handle* h, const int32_t* datapoints, int32_t B, int32_t accumulate, const int32_t* mask, int64_t nmask, int32_t mask_index_base,
#  float* grads, size_t n_grads, float* loss, float* losses)
WANT = [("mgn_handle", 1), ("i32", 1), ("i32", 0), ("i32", 0), ("i32", 1), ("i64", 0), ("i32", 0), ("f32", 1), ("size", 0), ("f32", 1),
        ("f32", 1)]
HEADER = os.path.join(os.path.dirname(js.JULIA_DIR), "include", "mgn_hip.h")


def test_declared_exported_and_bound(lib_built):
    hdr = open(HEADER).read()
    assert re.search(r"\bint\s+" + SYM + r"\s*\(", hdr)
    assert re.search(r"#define\s+MGN_DATAPOINT_BATCH_MAX\s+64\b", hdr)
    lib = _capi.load()
    assert hasattr(lib, SYM)
    ret, args = js.c_prototypes()[SYM]
    assert ret == ("i32", 0) and args == WANT
    restype, argtypes = _capi.PROTOTYPES[SYM]
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, i32p, C.c_int32, C.c_int32, i32p, C.c_int64, C.c_int32, f32p, C.c_size_t, f32p, f32p]


def test_abi_version_stands(lib_built):
    lib = _capi.load()
    lib.mgn_abi_version.restype = C.c_int
    assert lib.mgn_abi_version() == 4
    assert re.search(r"#define\s+MGN_ABI_VERSION\s+4\b", open(HEADER).read())


def test_python_classes():
    import mgn_amd
    assert callable(getattr(Engine, "step_datapoints"))
    assert not hasattr(mgn_amd.GroupEngine, "step_datapoints")        # no group form: the batched step drives one partition
    assert not any(name.startswith("mgn_group") and "datapoints" in name for name in _capi.PROTOTYPES)


def test_julia_binding():
    path = os.path.join(js.JULIA_DIR, "MGNHip.jl")
    text = js._strip_jl_comments(open(path).read())
    calls = [c for c in js.julia_ccalls(path) if c[0] == SYM]
    assert len(calls) == 1
    sym, ret, types, args = calls[0]
    assert len(types) == len(WANT) == len(args)
    assert js._compatible(js._JL[ret], ("i32", 0))
    for k, (t, c) in enumerate(zip(types, WANT)):
        assert js._compatible(js._JL[t], c), (k, t, c)
    assert re.search(r"^export\b[^\n]*\bstep_datapoints!", text, re.M)
    assert re.search(r"^function step_datapoints!\(", text, re.M)
    assert re.search(r"^const ABI_VERSION = 4\b", text, re.M)
