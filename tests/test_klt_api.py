"""The device-resident KLT tracker without a GPU: the six symbols are declared, exported and bound; the argument lists; the header states
the seven stages and what is out of scope; and every refusal that needs no device (the null context, the binding's own argument checks)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmv_klt_create", "pmv_klt_destroy", "pmv_klt_set_tracks", "pmv_klt_get_tracks", "pmv_klt_step", "pmv_debug_klt_stats"]
INVALID = -2


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def _code():
    return " ".join(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S).split())


def test_the_six_symbols_are_declared_exported_and_bound(pmv):
    code = _code()
    lib = pmv.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(\s*pmv_ctx\*" % name, code), f"{name} is not declared in include/pmv_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pmv.ABI_SYMBOLS
    for method in ("klt_create", "debug_klt_stats"):
        assert callable(getattr(pmv.Context, method))
    for method in ("step", "set_tracks", "get_tracks", "close"):
        assert callable(getattr(pmv.KltTracker, method))
    assert pmv.KLT_MAX_TRACKERS == 16 and "#define PMV_KLT_MAX_TRACKERS 16" in _header()


def test_the_declared_argument_lists():
    code = _code()
    assert "int pmv_klt_create(pmv_ctx* ctx, const pmv_klt_params* p, int* out_id);" in code
    assert "int pmv_klt_destroy(pmv_ctx* ctx, int id);" in code
    assert "int pmv_klt_set_tracks(pmv_ctx* ctx, int id, const int* ids, const int* ages, const float* xy, int n, int next_id);" in code
    assert "int pmv_klt_get_tracks(pmv_ctx* ctx, int id, int* ids, int* ages, float* xy, int cap, int* out_n);" in code
    assert ("int pmv_klt_step(pmv_ctx* ctx, int id, int prev_slot, int cur_slot, int* out_ids, int* out_ages, float* out_xy, float* out_prev_xy_or_null, "
            "int out_cap, int* out_n, int* out_counts8);") in code
    assert "int pmv_debug_klt_stats(pmv_ctx* ctx, long long* out4);" in code


def test_the_struct_is_the_headers(pmv):
    code = _code()
    body = code[code.index("typedef struct pmv_klt_params {"):code.index("} pmv_klt_params;")]
    fields = re.findall(r"(\w+)\s*(?:,\s*(\w+))?;", body.split("{", 1)[1])
    names = [n for pair in fields for n in pair if n]
    assert names == [f[0] for f in pmv.KltParams._fields_]
    p = pmv.klt_params()
    assert (p.target, p.border, p.fb_max_dist, p.reject_f, p.f_threshold, p.f_confidence, p.radius, p.subpix) == (150, 1, 0.5, 1, 1.0, 0.99, 10, 0)
    assert (p.gftt.quality, p.gftt.min_dist, p.gftt.block_size, p.gftt.use_harris) == (0.01, 10.0, 3, 0)
    assert pmv.klt_params(fb_max_dist=None).fb_max_dist < 0
    sig = inspect.signature(pmv.KltTracker.step)
    assert list(sig.parameters)[1:] == ["prev_slot", "cur_slot"]


def test_the_header_states_the_stages_and_what_is_out_of_scope():
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())
    doc = text[text.index("A device-resident KLT tracker"):text.index("#define PMV_KLT_MAX_TRACKERS")]
    for phrase in ("1. Track", "2. Filter", "3. rejectWithF", "4. Thin", "5. Refill", "6. Refine", "7. Append",
                   "pmv_lk_track_fb(prev_slot, cur_slot, state xy, flags 0)", "round half to even", "without contraction", "thr2 = (float)(fb_max_dist * fb_max_dist)",
                   "n1 >= 15", "ALL go", "counts[5] = -1", "out_keep does not depend on max_corners", "ids next_id .. next_id + m - 1 and age 1",
                   "{n0, n1, n2, n3, m, f_found (-1 not run / 0 / 1), f_samples_drawn, 0}", "waits ONCE", "at most twice", "libm's pow and log",
                   "nothing is written, nothing is clamped, the state is unchanged", "a 17th tracker", "out_cap < target", "pmv_ctx_destroy frees the trackers",
                   "Not logged by pmv_record_enable"):
        assert phrase in doc, phrase
    scope = doc[doc.index("Out of scope:"):]
    for phrase in ("pmv_batch_klt_*", "a region or base mask", "an initial-flow prediction", "per-track radius", "LMedS or 8-point", "undistorting points before F",
                   "id wrap-around"):
        assert phrase in scope, phrase


def test_a_null_context_is_refused_by_every_new_call(pmv):
    lib = pmv.load_library()
    p = pmv.klt_params()
    out = np.full(4, -7, np.int32)
    fl = np.full(4, -7, np.float32)
    vp, ci = C.c_void_p, C.c_int
    lib.pmv_klt_create.argtypes = [vp, vp, vp]
    lib.pmv_klt_destroy.argtypes = [vp, ci]
    lib.pmv_klt_set_tracks.argtypes = [vp, ci, vp, vp, vp, ci, ci]
    lib.pmv_klt_get_tracks.argtypes = [vp, ci, vp, vp, vp, ci, vp]
    lib.pmv_klt_step.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp]
    lib.pmv_debug_klt_stats.argtypes = [vp, vp]
    o, f = out.ctypes.data, fl.ctypes.data
    assert lib.pmv_klt_create(None, C.cast(C.pointer(p), vp), o) == INVALID
    assert lib.pmv_klt_destroy(None, 0) == INVALID
    assert lib.pmv_klt_set_tracks(None, 0, o, o, f, 2, 0) == INVALID
    assert lib.pmv_klt_get_tracks(None, 0, o, o, f, 2, o) == INVALID
    assert lib.pmv_klt_step(None, 0, 0, 1, o, o, f, f, 2, o, o) == INVALID
    assert lib.pmv_debug_klt_stats(None, o) == INVALID
    assert (out == -7).all() and (fl == -7).all()
    lib.pmv_last_error.restype = C.c_char_p
    assert b"pmv_debug_klt_stats" in lib.pmv_last_error(None)


def test_the_binding_refuses_malformed_arrays_before_the_library(pmv):
    class Dummy:
        lib, h = None, None
    trk = pmv.KltTracker(Dummy(), 0, 10)
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        trk.set_tracks(np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros((3, 3), np.float32), 0)
    with pytest.raises(ValueError, match="one id and one age per track"):
        trk.set_tracks(np.zeros(2, np.int32), np.zeros(3, np.int32), np.zeros((3, 2), np.float32), 0)
    with pytest.raises(TypeError):
        pmv.klt_params(no_such_field=1)
