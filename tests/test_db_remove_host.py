"""The item removal's surface, without a device: the four entry points are declared in include/spiral_hip.h and in the Rust shim with
the same number of arguments, the library exports them, the Python methods exist with the documented signatures, and the calls that
must fail before they reach a device do."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT

SYMBOLS = {"sp_db_remove_items": 4, "sp_db_remove_range": 4, "sp_db_sparse_trim": 2, "sp_server_remove_items": 5}


def test_symbols_in_header_shim_and_library():
    import sdk_amd
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spiral_hip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    lib = C.CDLL(sdk_amd.library_path())
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        r = re.search(r"pub fn %s\s*\(([^;]*?)\)\s*-> c_int;" % name, rs, flags=re.S)
        assert r and len(r.group(1).split(",")) == n_args, name
        assert hasattr(lib, name), name
    for wrapper in ("pub fn remove_items(&mut self, indices: &[usize])", "pub fn remove_range(&mut self, item0: usize, count: usize)",
                    "pub fn trim(&mut self)", "pub fn remove_items(&self, indices: &[usize])"):
        assert wrapper in rs, wrapper


def test_python_methods():
    from sdk_amd import spiral
    D, S = spiral.Database, spiral.Server
    assert list(inspect.signature(D.remove_items).parameters) == ["self", "indices"]
    assert list(inspect.signature(D.remove_range).parameters) == ["self", "item0", "count"]
    assert inspect.signature(D.remove_range).parameters["count"].default is None
    assert list(inspect.signature(D.trim).parameters) == ["self"]
    assert list(inspect.signature(S.remove_items).parameters) == ["self", "db", "indices"]
    rep = inspect.signature(D.repair_from).parameters
    assert list(rep) == ["self", "src", "seed", "remove"] and rep["remove"].default is False
    assert "no format has a delete" not in D.repair_from.__doc__


def test_null_handles_are_refused_before_any_device_call():
    import sdk_amd
    lib = sdk_amd.lib()
    n = C.c_size_t(0xCCCC)
    idx = (C.c_size_t * 2)(0, 1)
    for call in (lambda: lib.sp_db_remove_items(None, idx, C.c_size_t(2), C.byref(n)),
                 lambda: lib.sp_db_remove_range(None, C.c_size_t(0), C.c_size_t(1), C.byref(n)),
                 lambda: lib.sp_db_sparse_trim(None, C.byref(n)),
                 lambda: lib.sp_server_remove_items(None, None, idx, C.c_size_t(2), C.byref(n))):
        n.value = 0xCCCC
        assert call() == -1 and n.value == 0
    assert lib.sp_db_remove_items(None, None, C.c_size_t(0), None) == -1
