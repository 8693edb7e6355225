"""CPU-side checks of the translation ABI (include/rp_mi355x.h, rp_nlhe_translate): the symbols exist, the enum has the header's
values, the args struct has the size the header states and the offsets of its ctypes mirror, the defaults are the documented ones, and
the arguments are refused in the documented order before a device is needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

from robopoker_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rp_mi355x.h")
CALLS = ("rp_nlhe_translate", "rp_nlhe_translate_device")


def test_symbols_exist():
    lib, text = _lib.load(), open(HEADER).read()
    for name in CALLS:
        assert re.search(r"RP_API\s+int\s+" + name + r"\s*\(", text) and hasattr(lib, name) and name in _lib.declared_symbols()
        assert len(_lib._SIGNATURES[name][1]) == 13
    assert re.search(r"RP_API\s+void\s+rp_nlhe_translate_args_default\s*\(", text) and hasattr(lib, "rp_nlhe_translate_args_default")


def test_enum_values_and_struct_layout(tmp_path):
    text = open(HEADER).read()
    m = re.search(r"typedef enum \{([^}]*)\} rp_translation_kind;", text)
    values = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in m.group(1).split(",")))
    assert values == {"RP_TRANSLATE_SNAP": 0, "RP_TRANSLATE_HARMONIC": 1, "RP_TRANSLATE_PHARGMAX": 2}
    assert _lib.TRANSLATE == {"snap": 0, "harmonic": 1, "phargmax": 2}
    m = re.search(r"\}\s*rp_nlhe_translate_args;\s*/\*\s*(\d+) bytes\s*\*/", text)
    assert m and int(m.group(1)) == 24 == C.sizeof(_lib.NlheTranslateArgs)
    offsets = {f: getattr(_lib.NlheTranslateArgs, f).offset for f, _ in _lib.NlheTranslateArgs._fields_}
    assert offsets == dict(seed=0, first_id=8, kind=16, reserved=17)
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    if cc is not None:
        src = tmp_path / "sizes.c"
        src.write_text('#include <stddef.h>\n#include "rp_mi355x.h"\n_Static_assert(sizeof(rp_nlhe_translate_args) == 24, "size");\n' +
                       "".join(f'_Static_assert(offsetof(rp_nlhe_translate_args, {f}) == {at}, "{f}");\n' for f, at in offsets.items()) +
                       '_Static_assert(RP_TRANSLATE_SNAP == 0 && RP_TRANSLATE_HARMONIC == 1 && RP_TRANSLATE_PHARGMAX == 2, "kinds");\n')
        subprocess.check_call([cc, "-std=c11", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)])


def test_defaults():
    a = _lib.NlheTranslateArgs(seed=7, first_id=9, kind=2, reserved=(C.c_uint8 * 7)(*[1] * 7))
    _lib.load().rp_nlhe_translate_args_default(C.byref(a))
    assert (a.seed, a.first_id, a.kind, list(a.reserved)) == (0, 0, 0, [0] * 7)
    _lib.load().rp_nlhe_translate_args_default(None)  # tolerated, like the other defaults


def test_arguments_are_refused_before_a_device_is_needed():
    lib = _lib.load()
    handle = C.c_void_p(8)  # never dereferenced: every refusal below comes first
    hands = (C.c_uint8 * 192)()
    outs = [None] * 7
    for name in CALLS:
        call = getattr(lib, name)
        good = _lib.NlheTranslateArgs()
        assert call(None, 1, C.byref(good), hands, None, None, *outs) == _lib.RP_ERR_INVALID and b"rp_nlhe_translate: NULL handle" in lib.rp_last_error()
        assert call(handle, 1, None, hands, None, None, *outs) == _lib.RP_ERR_INVALID and b"NULL args" in lib.rp_last_error()
        bad = _lib.NlheTranslateArgs(kind=3)
        assert call(handle, 1, C.byref(bad), hands, None, None, *outs) == _lib.RP_ERR_INVALID and b"kind 3" in lib.rp_last_error()
        assert call(handle, 0, C.byref(bad), None, None, None, *outs) == _lib.RP_ERR_INVALID  # even for an empty batch
        for at in range(7):
            bad = _lib.NlheTranslateArgs()
            bad.reserved[at] = 1
            assert call(handle, 1, C.byref(bad), hands, None, None, *outs) == _lib.RP_ERR_INVALID and b"reserved" in lib.rp_last_error()
        assert call(handle, 1, C.byref(good), None, None, None, *outs) == _lib.RP_ERR_INVALID and b"NULL hands" in lib.rp_last_error()
        assert call(handle, 0, C.byref(good), None, None, None, *outs) == _lib.RP_OK  # n = 0: no launch, no device
