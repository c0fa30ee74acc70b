"""The ctypes signatures binding.lib() types by hand against the prototypes of include/*.h, and the room loop
of the host calls (binding._room_call) against a fake call.  Neither needs a GPU.

A prototype and a signature agree when they have as many parameters and each parameter, and the return
value, falls in the same class: pointer, 64-bit integer, 32-bit integer, int, double (void for a return).
A `name[N]` parameter is a pointer, so are the CMP_TYPE, DESTROY_TYPE and PRINT_TYPE typedefs; size_t is 64
bits wide."""
import ctypes as C
import os
import re

import pytest

from aho_corasick_1975_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("acm.h", "acm_gpu.h", "acm_segment.h", "acm_score.h", "acm_index.h")
# their parameter lists hold parentheses (a function pointer spelt out), which the prototype pattern does not take
SKIPPED = {"acm_insert_end_of_keyword", "acm_foreach_keyword"}
PROTOTYPE = re.compile(r"([A-Za-z_][\w\s\*]*?)\b(acm_\w+)\s*\(([^()]*)\)\s*;")
POINTER_TYPEDEFS = {"CMP_TYPE", "DESTROY_TYPE", "PRINT_TYPE"}
WORD_CLASS = {"uint64_t": "64", "int64_t": "64", "size_t": "64", "uint32_t": "32", "unsigned": "32", "int": "int", "double": "double"}


def c_class(decl, is_return=False):
    """the class of a C declaration: a parameter with its name, or a return type"""
    decl = decl.strip()
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in decl.split() if w not in ("const", "extern", "struct")]
    if not is_return and len(words) > 1:
        words = words[:-1]                                          # the parameter's name
    if words == ["void"]:
        return "void"
    if words[0] in POINTER_TYPEDEFS:
        return "pointer"
    assert len(words) == 1 and words[0] in WORD_CLASS, "a type this test has no class for: %r" % decl
    return WORD_CLASS[words[0]]


def ctypes_class(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C.Array)):
        return "pointer"
    if t is C.c_double:
        return "double"
    if t is C.c_int:
        return "int"
    assert t in (C.c_uint32, C.c_uint64, C.c_size_t, C.c_int64), "a ctypes type this test has no class for: %r" % t
    return "64" if C.sizeof(t) == 8 else "32"


def prototypes():
    """{name: (class of the return value, [class of each parameter])} of every prototype the pattern takes"""
    found = {}
    for header in HEADERS:
        with open(os.path.join(ROOT, "include", header)) as f:
            text = f.read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
        for ret, name, params in PROTOTYPE.findall(text):
            params = [] if params.strip() in ("", "void") else [c_class(p) for p in params.split(",")]
            assert name not in found, "%s is declared twice" % name
            found[name] = (c_class(ret, is_return=True), params)
    return found


def signature(L, name):
    fn = getattr(L, name)
    assert fn.argtypes is not None, "%s has no argtypes" % name
    return ctypes_class(fn.restype), [ctypes_class(t) for t in fn.argtypes]


def mismatches(L, protos):
    return {name: (proto, signature(L, name)) for name, proto in protos.items() if signature(L, name) != proto}


def test_every_export_is_checked_or_skipped_by_name():
    protos = prototypes()
    functions = {name for name in binding.EXPORTS if name.startswith("acm_")}
    assert SKIPPED <= functions and not SKIPPED & set(protos)
    assert functions - set(protos) == SKIPPED
    assert set(protos) <= functions, "a prototype EXPORTS does not list: %s" % sorted(set(protos) - functions)


def test_signatures_agree_with_the_headers():
    assert mismatches(binding.lib(), prototypes()) == {}


def test_a_u32_typed_for_a_uint64_is_caught():
    """the check has teeth: one argument of a copy of the library object retyped from 64 to 32 bits is reported"""
    L = C.CDLL(binding.library_path())
    for name in ("acm_gpu_scan_host", "acm_gpu_device_count"):
        getattr(L, name).restype = getattr(binding.lib(), name).restype
        getattr(L, name).argtypes = list(getattr(binding.lib(), name).argtypes)
    protos = {name: prototypes()[name] for name in ("acm_gpu_scan_host", "acm_gpu_device_count")}
    assert mismatches(L, protos) == {}
    assert signature(L, "acm_gpu_device_count") == ("int", [])
    wrong = list(L.acm_gpu_scan_host.argtypes)
    at = wrong.index(C.c_uint64)
    wrong[at] = C.c_uint32
    L.acm_gpu_scan_host.argtypes = wrong
    assert list(mismatches(L, protos)) == ["acm_gpu_scan_host"]


OVERFLOW = binding.ACM_GPU_E_OVERFLOW


class FakeCall:
    """a call that needs room for `need` entries: overflows below it, reports it either way"""

    def __init__(self, needs):
        self.needs, self.caps = list(needs), []

    def __call__(self, cap):
        need = self.needs[min(len(self.caps), len(self.needs) - 1)]
        self.caps.append(cap)
        return (binding.ACM_GPU_OK if cap >= need else OVERFLOW), need, ("out", cap)


def test_room_loop_one_call_when_it_fits():
    call = FakeCall([10])
    assert binding._room_call(call, "fake", 16) == (("out", 16), 10, 16)
    assert call.caps == [16]


def test_room_loop_default_capacity_is_repeated_with_the_reported_size():
    call = FakeCall([40])
    assert binding._room_call(call, "fake", 16) == (("out", 40), 40, 40)
    assert call.caps == [16, 40]


def test_room_loop_explicit_capacity_raises():
    call = FakeCall([40])
    with pytest.raises(binding.ACMError) as e:
        binding._room_call(call, "fake_what", 16, fixed=True)
    assert e.value.code == OVERFLOW and str(e.value).startswith("fake_what:")
    assert call.caps == [16]


def test_room_loop_once_raises_on_a_second_overflow():
    call = FakeCall([40, 90])                                       # the second call needs more than the first reported
    with pytest.raises(binding.ACMError) as e:
        binding._room_call(call, "fake_what", 16)
    assert e.value.code == OVERFLOW and str(e.value).startswith("fake_what:")
    assert call.caps == [16, 40]


def test_room_loop_until_it_fits_keeps_going():
    call = FakeCall([40, 90, 200, 200])
    assert binding._room_call(call, "fake", 16, repeats=None) == (("out", 200), 200, 200)
    assert call.caps == [16, 40, 90, 200]


def test_room_loop_other_errors_are_raised_at_once():
    with pytest.raises(binding.ACMError) as e:
        binding._room_call(lambda cap: (binding.ACM_GPU_E_ARG, 0, None), "fake_what", 16, repeats=None)
    assert e.value.code == binding.ACM_GPU_E_ARG
