"""native.parse_header without a GPU and without the library: tiny header texts, one per class of slot, per formatting hazard and
per refusal, then include/tripled_hip.h itself -- the ctypes signatures and the limits of the bindings are derived from it."""
import ctypes
import os

import pytest

import tripled_amd  # noqa: F401
from tripled_amd import cloud, cloud_align, cloud_eval, cloud_normals, evaluate, native, odometry, render, resize

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tripled_hip.h")
P = ctypes.POINTER


def _sig(text, name="td_f"):
    return native.parse_header(text)[0][name]


# ---- 1. one prototype per class of slot: the exact ctypes object ----------------------------------------------------------------

@pytest.mark.parametrize("param,slot", [
    ("int n", ctypes.c_int), ("float a", ctypes.c_float), ("double tau", ctypes.c_double), ("long long M", ctypes.c_longlong),
    ("const float* tgt", ctypes.c_void_p), ("uint8_t* argmin", ctypes.c_void_p), ("void* workspace", ctypes.c_void_p),
    ("unsigned long long* payload", ctypes.c_void_p), ("const double* poses", ctypes.c_void_p),
    ("td_stream_t stream", ctypes.c_void_p),
    ("TD_HOST const double* K", P(ctypes.c_double)), ("TD_HOST const int* invert", P(ctypes.c_int)),
    ("TD_HOST const long long* strides", P(ctypes.c_longlong)), ("TD_HOST const float* scale6", P(ctypes.c_float)),
    ("TD_HOST const float* const* src", P(ctypes.c_void_p)), ("TD_HOST float* const* src_rgbx", P(ctypes.c_void_p)),
    ("TD_HOST void** dw", P(ctypes.c_void_p)),
])
def test_slot(param, slot):
    restype, argtypes = _sig("int td_f(int first, %s, int last);" % param)
    assert restype is ctypes.c_int and len(argtypes) == 3
    assert argtypes[0] is ctypes.c_int and argtypes[1] is slot and argtypes[2] is ctypes.c_int


def test_slots_are_the_objects_call_classifies_by():
    """native._plan sorts slots by identity."""
    _, argtypes = _sig("int td_f(const float* a, TD_HOST const float* const* b, int c, td_stream_t stream);")
    assert argtypes[0] is native._P and argtypes[1] is native._PTRARR and argtypes[2] is native._I and argtypes[3] is native._P


@pytest.mark.parametrize("ret,restype", [("int", ctypes.c_int), ("long long", ctypes.c_longlong), ("const char*", ctypes.c_char_p),
                                         ("const char *", ctypes.c_char_p)])
def test_return_types_and_void_list(ret, restype):
    assert _sig("%s td_f(void);" % ret) == (restype, [])
    assert _sig("%s td_f(int code);" % ret)[0] is restype


# ---- 2. formatting ---------------------------------------------------------------------------------------------------------------

def test_formatting():
    text = """
/* a block comment with a prototype in it: int td_fake(int x); */
#ifndef GUARD_H
#define GUARD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define TD_HOST
typedef void* td_stream_t;
// int td_fake2(int x);
int td_f(const float* tgt,   /* [B,3,H,W]; commas, (parentheses) and a ; in here */
         TD_HOST const float* const*
             src,
         int n_src,          // the rest of this line: int td_fake3(void);
         td_stream_t
         stream);
long long td_g( void );
#ifdef __cplusplus
}
#endif
#endif /* GUARD_H */
"""
    signatures, constants = native.parse_header(text)
    assert list(signatures) == ["td_f", "td_g"] and constants == {}
    assert signatures["td_f"] == (ctypes.c_int, [ctypes.c_void_p, P(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p])
    assert signatures["td_g"] == (ctypes.c_longlong, [])


# ---- 3. refusals: a prototype the parser cannot read is an error, never a missing entry -------------------------------------------

@pytest.mark.parametrize("text,names", [
    ("int td_f(unsigned n);", ("td_f", "n")),
    ("int td_f(int a, size_t n);", ("td_f", "n")),
    ("int td_f(const float** src);", ("td_f", "src")),                       # no device arrays of pointers: TD_HOST is missing
    ("int td_f(float* const* src, int n);", ("td_f", "src")),
    ("int td_f(TD_HOST int n);", ("td_f", "n")),
    ("int td_f(TD_HOST const uint8_t* lut);", ("td_f", "lut")),
    ("int td_f(TD_HOST const void* x);", ("td_f", "x")),
    ("int td_f(const float*);", ("td_f", "const float*")),                 # a parameter without a name
    ("int td_f();", ("td_f",)),
    ("void td_f(int n);", ("td_f",)),                                       # a return type outside the map
    ("unsigned td_f(int n);", ("td_f",)),
    ("int td_table[4];", ("td_table",)),                                    # a declaration that is no prototype
    ("struct td_s { int a; };", ("td_s",)),
    ("int td_f(int (*callback)(int));", ("td_f",)),
    ("int td_f(int a)\nint td_g(int b);", ("td_f", "td_g")),                 # a missing ';', caught through the next declaration
    ("int td_g(int b);\nint td_f(int a)", ("td_f",)),                        # ... and at the end of the file
    ("int td_f(int a);\nint td_f(int a, int b);", ("td_f",)),                # declared twice
    ("#define TD_A (1 << 3)\n", ("TD_A",)),
    ("#define TD_A 0x10\n", ("TD_A",)),
])
def test_refusals_name_the_offender(text, names):
    with pytest.raises(ValueError) as e:
        native.parse_header(text)
    for name in names:
        assert name in str(e.value), str(e.value)


# ---- 4. constants ----------------------------------------------------------------------------------------------------------------

def test_constants():
    text = """
#define TD_A 3
#define TD_B (-1)      /* in parentheses */
#define TD_C 0.5009765625 // 1/2 + 2^-10
  #  define   TD_D   16
#define TD_HOST
#define GUARD_H
#define NOT_OURS 7
/* #define TD_E 5 */
// #define TD_F 6
int td_f(void);
"""
    constants = native.parse_header(text)[1]
    assert constants == {"TD_A": 3, "TD_B": -1, "TD_C": 0.5 + 2.0 ** -10, "TD_D": 16}
    assert [type(constants[k]) for k in ("TD_A", "TD_B", "TD_C")] == [int, int, float]


# ---- 5. the real header ----------------------------------------------------------------------------------------------------------

SCALARS = (ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong, ctypes.c_void_p)


def test_real_header():
    signatures, constants = native.parse_header(open(HEADER).read())
    assert len(signatures) >= 115 and all(name.startswith("td_") for name in signatures)
    assert signatures.keys() == native.SIGNATURES.keys()
    for name, (restype, argtypes) in signatures.items():      # the table in use is this parse, object for object
        assert restype is native.SIGNATURES[name][0] and len(argtypes) == len(native.SIGNATURES[name][1]), name
        assert all(a is b for a, b in zip(argtypes, native.SIGNATURES[name][1])), name
    host = [(name, i) for name, (_, argtypes) in signatures.items() for i, a in enumerate(argtypes) if a not in SCALARS]
    assert len(host) == 45, host      # the TD_HOST parameters: a forgotten or surplus mark moves this number
    host_types = {signatures[name][1][i] for name, i in host}
    assert host_types == {P(ctypes.c_void_p), P(ctypes.c_int), P(ctypes.c_longlong), P(ctypes.c_double), P(ctypes.c_float)}
    assert constants == native.CONSTANTS
    assert native.ABI_VERSION == 3 and native.TD_MAX_SRC == 4
    assert sorted(native.DTYPE_CODES.values()) == [0, 1]


def test_limits_keep_their_values():
    """The limits a caller sizes buffers and host arrays by, pinned here and not by a comment beside a copy."""
    got = (render.MAX_SPLAT, render.MAX_SURFEL, render.SURFEL_SLACK, cloud.MAX_VIEW_RADIUS, cloud_eval.MAX_THRESHOLDS, resize.MAX_SIZES,
           cloud_align.SLOTS, cloud_align.PLANE_SLOTS, cloud_normals.SWEEPS, odometry.MAX_LENGTHS, odometry.TRAJECTORY_THREADS,
           evaluate.STEREO_SCALE_FACTOR)
    assert got == (8, 16, 0.5009765625, 8, 16, 16, 17, 37, 4, 16, 256, 36)
    assert [type(v) for v in got] == [int, int, float] + [int] * 9
    assert render.SURFEL_SLACK == 0.5 + 2.0 ** -10
    c = native.CONSTANTS
    assert got == (c["TD_RENDER_MAX_SPLAT"], c["TD_SURFEL_MAX"], c["TD_SURFEL_SLACK"], c["TD_VIEWS_MAX_RADIUS"],
                   c["TD_NN_MAX_THRESHOLDS"], c["TD_RESIZE_MAX_SIZES"], c["TD_ICP_SLOTS"], c["TD_ICP_PLANE_SLOTS"],
                   c["TD_NORMALS_SWEEPS"], c["TD_ODOM_MAX_LENGTHS"], c["TD_ODOM_THREADS"], c["TD_STEREO_SCALE_FACTOR"])


# ---- 6. arity ----------------------------------------------------------------------------------------------------------------------

def test_call_counts_against_the_header(monkeypatch):
    """One argument too few is a TypeError before the library is loaded: the count is the header's."""
    def no_load(path=None):
        raise AssertionError("the library must not be loaded")
    monkeypatch.setattr(native, "load", no_load)
    assert len(native.SIGNATURES["td_cloud_transform"][1]) == 7      # src, N, c, R, t, out, stream
    R, t = (ctypes.c_double * 9)(), (ctypes.c_double * 3)()
    with pytest.raises(TypeError, match="td_cloud_transform takes 6 arguments in front of the stream, got 5"):
        native.call("td_cloud_transform", None, 0, 1.0, R, t)
    with pytest.raises(TypeError, match="got 7"):
        native.call("td_cloud_transform", None, 0, 1.0, R, t, None, None)
