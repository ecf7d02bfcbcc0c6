"""The host builds of the tests: tests/<dir>/<dir>.cpp, which restates kernels as serial loops over one of the math headers of
mpmavatar_amd/csrc, compiled with g++ over the stand-in for the HIP runtime (tests/hostmath/stub) into tests/<dir>/_build/.
Test infrastructure only.

A target is rebuilt when it is older than its source, ANY header of mpmavatar_amd/csrc or the stub: no list of the headers a
source happens to include, so a nested include cannot be forgotten and a stale library cannot be compared against new
device code.  The price is a rebuild of about a second each after an unrelated header changes."""
import ctypes as C
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mpmavatar_amd", "csrc")
STUB = os.path.join(HERE, "hostmath", "stub")
_loaded = {}


def _compile(source, target, flags):
    src = os.path.join(HERE, source, source + ".cpp")
    out = os.path.join(HERE, source, "_build", target)
    deps = [src] + glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(STUB, "**", "*"), recursive=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-I", STUB, "-I", CSRC, *flags, src, "-o", out])
    return out


def host_lib(source, *, name=None, flags=()):
    """tests/<source>/<source>.cpp as a shared library, loaded once per path -> ctypes.CDLL.  flags come after the shared
    ones and win over them (the contraction variants of test_hip_math_on_host.py); name tells such variants apart."""
    path = _compile(source, f"lib{name or source}.so", ["-O2", "-fPIC", "-shared", *flags])
    if path not in _loaded:
        _loaded[path] = C.CDLL(path)
    return _loaded[path]


def host_program(source, *, name, flags=()):
    """the same file as a stand-alone program (the source's own main) -> its path, for a subprocess; nothing is loaded"""
    return _compile(source, name, flags)
