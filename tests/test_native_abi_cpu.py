"""The declaration table of _native.lib() held against include/fq.h, on a box without a GPU.

lib() declares every entry point of libfq_hip.so by position (`[vp, vp, vp, vp] + [ci] * 19 + [vp]`); ctypes converts what it is
told to, so a row one `ci` short or a `size_t` declared `c_int` passes garbage silently.  Here every `fq_*` prototype of the header
(comments stripped, prototypes span lines) is compared with the restype / argtypes found on the loaded library: the same names on
both sides, the same return type, and position by position the same class of argument -- a pointer or fq_stream_t against
c_void_p / c_char_p / POINTER(...), int against c_int, size_t against c_size_t, long against c_long, float against c_float.  The
rows lib() derives in loops (the `_act` siblings) are checked like any other.  The header is the contract: where the two
disagree, the table row is what is wrong."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPE = re.compile(r"\b(int|size_t|const\s+char\s*\*)\s*(fq_\w+)\s*\(([^()]*)\)\s*;")
RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
VALUES = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long": ctypes.c_long, "float": ctypes.c_float}


def _arg_class(decl):
    """'ptr', or the ctypes type of a by-value parameter declaration such as `int rs_min` or `size_t n`."""
    if "*" in decl or re.match(r"(const\s+)?fq_stream_t\b", decl):
        return "ptr"
    words = decl.replace("const ", "").split()
    assert len(words) == 2 and words[0] in VALUES, "a parameter this test has no rule for: %r" % decl
    return VALUES[words[0]]


def _ctypes_class(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "ptr"
    return t


def header_prototypes():
    """{name: (restype, [argument class, ...])} of every fq_* prototype in include/fq.h"""
    with open(os.path.join(ROOT, "include", "fq.h")) as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    out = {}
    for ret, name, params in PROTOTYPE.findall(text):
        assert name not in out, "declared twice: " + name
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (RETURNS[re.sub(r"\s*\*", "*", " ".join(ret.split()))], [] if params == ["void"] else [_arg_class(p) for p in params])
    return out


@pytest.fixture(scope="module")
def bound():
    """{name: function} of what a fresh lib() touches on the library it loads (ctypes keeps every function looked up on a CDLL in
    its __dict__; a fresh load, so that nothing another test looked up is counted)."""
    from common.quantity import _native
    before = _native._lib
    _native._lib = None
    try:
        L = _native.lib()
    finally:
        _native._lib = before
    return dict((n, f) for n, f in vars(L).items() if n.startswith("fq_"))


def _exported():
    """The fq_* names the shared library exports (nm -D --defined-only), without the fq_debug_* probes."""
    from common.quantity import _native
    nm = shutil.which("nm") or shutil.which("llvm-nm") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-nm")
    txt = subprocess.run([nm, "-D", "--defined-only", _native.LIB_PATH], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    names = set(line.split()[-1] for line in txt.splitlines() if line.split())
    return set(n for n in names if n.startswith("fq_") and not n.startswith("fq_debug_"))


def test_every_prototype_is_bound_and_every_bound_name_is_in_the_header(bound):
    protos = header_prototypes()
    assert sorted(set(protos) - set(bound)) == [], "in fq.h, not declared by lib()"
    assert sorted(set(bound) - set(protos)) == [], "declared by lib(), not in fq.h"
    assert len(protos) == len(bound)
    exported = _exported()
    assert len(protos) >= len(exported), sorted(exported - set(protos))      # a parser that skips prototypes fails here
    assert sorted(set(protos) - exported) == [], "in fq.h, not exported by the library"


def test_restype_and_argtypes_match_the_header_position_by_position(bound):
    protos = header_prototypes()
    wrong = []
    for name in sorted(set(protos) & set(bound)):
        ret, args = protos[name]
        fn = bound[name]
        if fn.restype is not ret:
            wrong.append("%s: restype %r, the header returns %r" % (name, fn.restype, ret))
        if fn.argtypes is None:
            if args:                                                          # (a `void` prototype may go without)
                wrong.append("%s: no argtypes for %d parameters" % (name, len(args)))
            continue
        got = [_ctypes_class(t) for t in fn.argtypes]
        if len(got) != len(args):
            wrong.append("%s: %d argtypes for %d parameters" % (name, len(got), len(args)))
            continue
        wrong += ["%s: argument %d is %r, the header has %r" % (name, i, g, a) for i, (g, a) in enumerate(zip(got, args)) if g != a]
    assert wrong == []


def test_the_parser_reads_the_forms_the_header_uses():
    protos = header_prototypes()
    assert protos["fq_version"] == (ctypes.c_int, [])
    assert protos["fq_status_string"] == (ctypes.c_char_p, [ctypes.c_int])
    assert protos["fq_kl_workspace_bytes_n"] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
    ret, args = protos["fq_block_tail_i8"]                                     # spans lines; the one `long`
    assert ret is ctypes.c_int and len(args) == 23 and args[18] is ctypes.c_long and args[-1] == "ptr"
    assert protos["fq_conv1x1_f32_act"][1][5] is ctypes.c_float
