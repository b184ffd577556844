"""The C-ABI extension headers (openpystruct_amd/_cabi.py EXTENSION_HEADER_PATHS) under the checks tests/test_cabi.py makes of the main
header: every prototype they declare is exported by the built library and bound with checked argument types, and a C++ compiler that
includes the real headers agrees with the ctypes types the binding derived."""
import os
import re
import shutil
import subprocess

import pytest

from openpystruct_amd import _cabi, build
from tests.test_cabi import _REFEREE, _kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extension_symbols_are_exported_and_bound():
    build.build()
    lib = _cabi.load()
    assert _cabi.EXTENSION_EXPORTS and not set(_cabi.EXTENSION_EXPORTS) & set(_cabi.EXPORTS)
    for path, abi in _cabi._extensions.items():
        hdr = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        declared = set(re.findall(r"\b(ops_[a-z0-9_]+)\s*\(", hdr))
        assert declared == set(abi.functions), path
        for name in declared:
            assert getattr(lib, name).argtypes == abi.functions[name][1] and getattr(lib, name).restype is abi.functions[name][0], name
    assert {"ops_frame_adjoint_rhs_f64", "ops_frame_grad_contract_f64"} <= set(_cabi.EXTENSION_EXPORTS)


def test_extension_bindings_agree_with_the_compiler(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found: the referee program cannot be built")
    for path, abi in _cabi._extensions.items():
        calls = "".join(f"  FUNC({name});\n" for name in abi.functions)
        text = _REFEREE.replace('#include "openpystruct_amd.h"', f'#include "openpystruct_amd.h"\n#include "{os.path.basename(path)}"')
        src, exe = tmp_path / "referee.cpp", tmp_path / "referee"
        src.write_text(text.replace("@CALLS@", calls))
        subprocess.check_call(["g++", "-std=c++17", "-I", os.path.dirname(path), "-o", str(exe), str(src)])
        seen = {}
        for line in subprocess.check_output([str(exe)], text=True).splitlines():
            tag, name, *rest = line.split()
            assert tag == "F"
            seen[name] = rest
        assert set(seen) == set(abi.functions)
        for name, (restype, argtypes) in abi.functions.items():
            assert seen[name] == [_kind(restype)] + [_kind(t) for t in argtypes], name
