"""The kernel library's C interface is written down once, in
csrc/kernels/beekern.h; this checks the copies against it, without a GPU and
without loading the library into Python:

* ``_native.SIGNATURES`` (the ctypes binding) against the header's declarations;
* the symbols the built library exports against the header's, both ways;
* the Python side's limits against the header's constants;
* the size of every ticketed workspace against the numbers of the per-kernel
  exports that bk_workspace_bytes replaced -- a workspace smaller than its
  kernel expects would be an out-of-bounds write on the GPU -- through a small
  program of its own (tests/native_abi_main.cpp) linked against the library.

And the launch dispatch the kernel files share (csrc/kernels/bk_dispatch.hpp), through a
program of its own (tests/dispatch_main.cpp) built by g++ with sanitizers."""

import ctypes
import os
import re
import subprocess

import pytest

from bee_code_interpreter_fs_amd import _build
from bee_code_interpreter_fs_amd.ops import _native
from bee_code_interpreter_fs_amd.ops import driver as drvmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "csrc", "kernels", "beekern.h")
# exports that Python does not bind (the kernel broker calls them)
NOT_BOUND = ("bk_reserve",)
OLD_WORKSPACE_EXPORTS = tuple(f"bk_{k}_workspace_{what}" for k in ("reduce", "reduce_axis", "axis_stat", "compress",
                                                                   "select", "histogram") for what in ("bytes", "init"))
# bk_workspace_bytes by kind.  The first four follow from the layouts
# (reduce.hip, axis.hip, mask.hip); the last two are sizeof(SelectWs) and
# sizeof(HistWs) of stats.hip, as the select and the histogram size export of
# the last build that had them returned them
WORKSPACE_BYTES = [32768 * 8 + 256, (1 << 18) * 8 + 4096 * 4, 2 * (1 << 18) * 8 + 4096 * 4, 2 * 2048 * 8 + 256, 66560,
                   33024]
SCALARS = {"int": "i32", "int64_t": "i64", "uint64_t": "u64", "float": "f32", "double": "f64"}
CTYPES = {ctypes.c_int: "i32", ctypes.c_int64: "i64", ctypes.c_uint64: "u64", ctypes.c_float: "f32",
          ctypes.c_double: "f64", ctypes.c_void_p: "ptr", ctypes.c_char_p: "ptr"}


def _header_text():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _c_kind(decl, named):
    """The class of a C type; ``named``: the declarator ends with the argument's name."""
    if "*" in decl or "hipStream_t" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    if named:
        assert len(words) == 2, f"an argument without a name: {decl!r}"
        words = words[:1]
    assert len(words) == 1 and words[0] in SCALARS, decl
    return SCALARS[words[0]]


@pytest.fixture(scope="module")
def declared():
    """name -> (argument classes, result class) of every BK_API declaration of the header."""
    out = {}
    for body in re.findall(r"^BK_API\s+([^;]*);", _header_text(), flags=re.M):
        m = re.fullmatch(r"(.*?)\b(bk_\w+)\s*\((.*)\)", " ".join(body.split()))
        assert m, body
        result, name, args = m.groups()
        assert name not in out, name
        args = [a.strip() for a in args.split(",")] if args.strip() not in ("", "void") else []
        out[name] = ([_c_kind(a, True) for a in args], _c_kind(result, False))
    assert len(out) > 50
    return out


@pytest.fixture(scope="module")
def constants():
    """The header's enumerators: written values, and positions in enum BkWorkspace."""
    text = _header_text()
    values = {name: int(eval(expr, {"__builtins__": {}})) for name, expr in re.findall(r"\b(BK_MAX_\w+)\s*=\s*([^,}\n]+)", text)}
    kinds = re.search(r"enum\s+BkWorkspace\s*\{([^}]*)\}", text).group(1)
    for i, name in enumerate(n.strip().split("=")[0].strip() for n in kinds.split(",") if n.strip()):
        values[name] = i
    return values


@pytest.fixture(scope="module")
def library():
    return _build.build(["beekern"], verbose=False)[0]


def _py_kind(t):
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return "ptr"
    return CTYPES[t]


def test_signatures_match_the_header(declared):
    for name, (args, result) in _native.SIGNATURES.items():
        assert name in declared, f"{name} is bound in _native.py but not declared in beekern.h"
        assert ([_py_kind(a) for a in args], _py_kind(result)) == declared[name], name
    unbound = sorted(set(declared) - set(_native.SIGNATURES))
    assert unbound == sorted(NOT_BOUND)


def test_exports_match_the_header(declared, library):
    out = subprocess.run(["nm", "-D", "--defined-only", library], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("bk_")}
    assert exported == set(declared), (sorted(exported - set(declared)), sorted(set(declared) - exported))
    assert not exported & set(OLD_WORKSPACE_EXPORTS)


def test_python_limits_match_the_header(constants):
    import importlib

    array = importlib.import_module("bee_code_interpreter_fs_amd.ops.array")  # (ops.array is also a function)
    assert drvmod.MAX_RANKS == constants["BK_MAX_RANKS"]
    assert drvmod.MAX_BINS == array.MAX_HISTOGRAM_BINS == constants["BK_MAX_BINS"]
    assert array.MAX_AXIS0_COLUMNS == constants["BK_MAX_AXIS0_COLUMNS"]
    assert [drvmod.WS_REDUCE, drvmod.WS_REDUCE_AXIS, drvmod.WS_AXIS_STAT, drvmod.WS_COMPRESS, drvmod.WS_SELECT,
            drvmod.WS_HISTOGRAM, drvmod.WS_COUNT] == [constants[k] for k in (
                "BK_WS_REDUCE", "BK_WS_REDUCE_AXIS", "BK_WS_AXIS_STAT", "BK_WS_COMPRESS", "BK_WS_SELECT",
                "BK_WS_HISTOGRAM", "BK_WS_COUNT")]


def test_workspace_sizes_are_the_replaced_exports(library, tmp_path):
    prog = str(tmp_path / "native_abi_main")
    libdir = os.path.dirname(library)
    rocm_lib = os.path.join(_build.ROCM, "lib")
    subprocess.run([_build.CXX, "-std=c++17", "-Wall", "-Wextra", f"-I{_build.ROCM}/include", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "native_abi_main.cpp"), "-o", prog, f"-L{libdir}", "-lbeekern",
                    f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rocm_lib}", f"-Wl,-rpath-link,{rocm_lib}"],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([prog], capture_output=True, text=True, check=True, timeout=60).stdout
    lines = [line.split() for line in out.splitlines()]
    assert lines[0] == ["count", str(len(WORKSPACE_BYTES))]
    got = {int(k): int(v) for what, k, v in (p for p in lines if p[0] == "bytes")}
    assert got == {-1: 0, len(WORKSPACE_BYTES): 0, **dict(enumerate(WORKSPACE_BYTES))}
    # unknown kinds and a null workspace: kBadArgument (1), answered before any HIP call
    assert [p for p in lines if p[0].startswith("init")] == [["init", "-1", "1"], ["init", str(len(WORKSPACE_BYTES)), "1"],
                                                             ["init_null", "1"]]


def test_launch_dispatch_reaches_one_instantiation(tmp_path):
    """csrc/kernels/bk_dispatch.hpp alone, as plain C++ under ASan / UBSan (tests/dispatch_main.cpp checks
    each call itself): an op, flag or dtype code reaches its one instantiation, any other is kBadArgument."""
    prog = str(tmp_path / "dispatch_main")
    subprocess.run([_build.CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", os.path.join(ROOT, "tests", "dispatch_main.cpp"), "-o", prog],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([prog], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout == "dispatch ok\n", run.stdout + run.stderr
