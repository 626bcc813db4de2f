"""pmv_set_lk_params without a GPU: the three symbols are declared, exported and bound; the ctypes mirror of pmv_lk_params has the header's
fields, types and C layout; the binding hands its keyword arguments to the library as that struct; the header states the contract; the
product library still links nothing from oracle/."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmv_set_lk_params", "pmv_get_lk_params", "pmv_debug_lk_general"]
CTYPES = {"int": C.c_int, "double": C.c_double, "float": C.c_float}


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def test_the_new_symbols_are_declared_exported_and_bound(pmv):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = pmv.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(\s*pmv_ctx\*" % name, code), f"{name} is not declared in include/pmv_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pmv.ABI_SYMBOLS
    for method in ("set_lk_params", "lk_params", "debug_lk_general"):
        assert callable(getattr(pmv.Context, method))


def test_struct_layout_matches_the_header(pmv):
    """same field names and C types in the same order; the offsets are those a C compiler gives the header's struct (natural alignment)"""
    src = _header()
    body = src[src.index("typedef struct pmv_lk_params {"):src.index("} pmv_lk_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"\b(int|double|float)\s+(\w+)\s*;", body)
    assert [(n, CTYPES[t]) for t, n in decl] == list(pmv.LKParams._fields_)
    off = 0
    for t, n in decl:
        size = C.sizeof(CTYPES[t])
        off = (off + size - 1) // size * size
        assert getattr(pmv.LKParams, n).offset == off, n
        off += size
    assert C.sizeof(pmv.LKParams) == (off + 7) // 8 * 8 == 32


def test_the_header_states_the_defaults_the_binding_uses(pmv):
    src = _header()
    body = src[src.index("typedef struct pmv_lk_params {"):src.index("} pmv_lk_params;")]
    stated = dict(re.findall(r"(\w+);\s*/\*.*?default ([0-9.e-]+)f? \*/", body))
    import inspect
    sig = inspect.signature(pmv.Context.set_lk_params)
    assert {k: float(v) for k, v in stated.items()} == {k: float(p.default) for k, p in sig.parameters.items() if k != "self"}


class _Recorder:
    """stands in for the library: records the arguments of every call and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        class _Fn:
            argtypes = None

            def __call__(fn, *args):
                self.calls.append((name, args))
                return 0
        f = _Fn()
        object.__setattr__(self, name, f)
        return f


def test_the_binding_passes_the_struct(pmv):
    ctx = object.__new__(pmv.Context)
    ctx.lib, ctx.h = _Recorder(), None
    ctx.set_lk_params(win=21, max_level=3, max_iter=20, eps=0.03, min_eig=1e-3)
    name, args = ctx.lib.calls[0]
    p = C.cast(args[1], C.POINTER(pmv.LKParams)).contents
    assert name == "pmv_set_lk_params" and (p.win, p.max_level, p.max_iter, p.eps) == (21, 3, 20, 0.03) and abs(p.min_eig - 1e-3) < 1e-9
    ctx.debug_lk_general(True)
    assert ctx.lib.calls[1] == ("pmv_debug_lk_general", (None, 1))


def test_the_header_states_the_contract():
    src = " ".join(_header().replace("*", " ").split())
    doc = src[src.index("OpenCVLucasKanadeFM.h:9-10"):src.index("typedef struct pmv_lk_params")]
    for phrase in ("3 <= win <= 63", "0 <= max_level <= 4", "1 <= max_iter <= 100", "0 <= eps <= 10", "min_eig >= 0 and finite", "nothing is clamped",
                   "EMPTIES EVERY FRAME SLOT", "contents are lost", "before pmv_batch_open", "pmv_frames_stream_begin bracket", "non-square windows",
                   "OPTFLOW_USE_INITIAL_FLOW", "OPTFLOW_LK_GET_MIN_EIGENVALS"):
        assert phrase in doc, phrase


def test_product_library_still_links_nothing_from_the_oracle(pmv):
    assert "liborc" not in subprocess.check_output(["ldd", pmv.lib_path()], text=True)
    assert " orc_" not in subprocess.check_output(["nm", "-D", "--defined-only", pmv.lib_path()], text=True)
