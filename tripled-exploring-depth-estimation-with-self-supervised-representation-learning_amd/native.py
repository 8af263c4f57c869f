"""ctypes binding of libtripled_hip.so (C ABI: include/tripled_hip.h).

There is deliberately no fallback: if the shared library is missing or a call returns an
error code, an exception is raised.  Nothing in here touches ``oracle/``.
"""
import ctypes
import functools
import os
import re

import torch

from . import dispatch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtripled_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "tripled_hip.h")


class NativeLibraryError(RuntimeError):
    pass


_I, _P = ctypes.c_int, ctypes.c_void_p
_PTRARR = ctypes.POINTER(ctypes.c_void_p)      # a TD_HOST array of device pointers
_SCALARS = {"int": _I, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong}
_RETURNS = {"int": _I, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p}


@functools.lru_cache(maxsize=None)
def _slot(ctype):
    """The ctypes type of a parameter type of the header (the closed map of parse_header); None for anything outside it."""
    words = ctype.replace("*", " * ").split()
    host, stars = words[:1] == ["TD_HOST"], words.count("*")
    base = " ".join(w for w in words[host:] if w not in ("const", "*"))
    if not base:
        return None
    if host:      # a typed host array, or a host array of device pointers
        return _PTRARR if stars == 2 else ctypes.POINTER(_SCALARS[base]) if stars == 1 and base in _SCALARS else None
    if stars == 0:
        return _P if base == "td_stream_t" else _SCALARS.get(base)
    return _P if stars == 1 else None      # a device pointer or an opaque workspace, whatever it points to; never a T**


def parse_header(text):
    """include/tripled_hip.h -> ({entry point: (restype, argtypes)}, {TD_NAME: number}): the ONE statement of the C ABI, read, not
    restated.  Not a C parser: it knows the few forms the header uses and raises ValueError on anything else, so a prototype it
    cannot read is never a missing entry.  Constants: ``#define TD_NAME literal`` (an integer, bare or in parentheses, or a decimal
    floating literal; a define without a value is ignored).  Types: int / float / double / long long scalars, td_stream_t and any
    unmarked ``T*`` -> c_void_p (a device pointer), ``TD_HOST T* const*`` -> POINTER(c_void_p), ``TD_HOST const T*`` with T one of
    the four scalars -> POINTER(c_T); an unmarked ``T**`` is an error (there are no device arrays of pointers).  Returns int,
    long long or const char*.  Parameters are written ``type name``, the stars with the type."""
    text = re.sub(r"/\*[^*]*\*+(?:[^/*][^*]*\*+)*/|//[^\n]*", " ", text)      # comments (the unrolled form of /\*.*?\*/: 5x faster)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(TD_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        m = re.fullmatch(r"\(\s*(-?\d+)\s*\)|(-?\d+)|(-?\d+\.\d+)", value)
        if not m:
            raise ValueError("#define %s %s: the value is not an integer or decimal literal" % (name, value))
        constants[name] = float(m.group(3)) if m.group(3) else int(m.group(1) or m.group(2))
    # the lines of the preprocessor, of the extern "C" braces and of typedefs go; what is left is prototypes, each closed by its ';'
    text = re.sub(r'^[ \t]*(?:#.*|\}|extern[ \t]+"C"[ \t]*\{|typedef\b[^;\n]*;)[ \t]*$', "", text, flags=re.M)
    *declarations, rest = " ".join(text.split()).split(";")
    if rest:
        raise ValueError("not a prototype (no terminating ';'): %r" % rest)
    signatures = {}
    for decl in declarations:
        m = re.fullmatch(r" ?(.*?) ?\b(\w+) ?\(([^()]*)\) ?", decl)
        ret = m and m.group(1).replace(" *", "*")
        if not m or ret not in _RETURNS or m.group(2) in signatures:
            raise ValueError("not a prototype this binding can read: %r" % decl.strip())
        name, params = m.group(2), m.group(3).strip()
        if not params:
            raise ValueError("%s: an empty parameter list; write (void)" % name)
        argtypes = []
        for param in [] if params == "void" else params.split(","):
            ctype, _, pname = param.strip().rpartition(" ")
            slot = _slot(ctype) if pname.isidentifier() else None
            if slot is None:
                raise ValueError("%s: parameter %r is outside the types this binding reads (int, float, double, long long, "
                                 "td_stream_t, T*, TD_HOST T* const*, TD_HOST const int / long long / float / double*)"
                                 % (name, param.strip()))
            argtypes.append(slot)
        signatures[name] = (_RETURNS[ret], argtypes)
    return signatures, constants


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise NativeLibraryError("include/tripled_hip.h not found at %s (%s) -- the ctypes signatures and the limits of the "
                                 "bindings are derived from it; there is no restated copy" % (HEADER_PATH, e)) from e


# name -> (restype, argtypes), and the header's numeric #defines: derived once per process, never written down here
SIGNATURES, CONSTANTS = parse_header(_read_header())
ABI_VERSION = CONSTANTS["TD_ABI_VERSION"]
TD_MAX_SRC = CONSTANTS["TD_MAX_SRC"]
DTYPE_CODES = {torch.float32: CONSTANTS["TD_DTYPE_F32"], torch.bfloat16: CONSTANTS["TD_DTYPE_BF16"]}

_lib = None


def load(path=None):
    """Load (once) and return the ctypes handle; raises NativeLibraryError if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("TD_HIP_LIB") or LIB_PATH      # TD_HIP_LIB: alternative build of the same ABI
    if not os.path.exists(path):
        raise NativeLibraryError(
            "libtripled_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C <package>/csrc`; there is no non-HIP fallback" % path)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise NativeLibraryError("cannot load %s: %s" % (path, e)) from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise NativeLibraryError("%s does not export %s" % (path, name)) from e
        fn.restype = res
        fn.argtypes = args
    if lib.td_abi_version() != ABI_VERSION:
        raise NativeLibraryError("ABI version mismatch: library %d, binding %d" % (lib.td_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(code, what):
    dispatch.hip(what)
    if code != 0:
        lib = load()
        msg = lib.td_error_string(code).decode()
        # the record holds the last failed LAUNCH of this thread, whichever call that was: it explains TD_ERR_LAUNCH and nothing else
        hip = lib.td_last_hip_error().decode() if code == CONSTANTS["TD_ERR_LAUNCH"] else ""
        raise NativeLibraryError("%s failed: %s (%d)%s" % (what, msg, code, (" [" + hip + "]") if hip else ""))


def require_device(*tensors):
    """The guard of every kernel wrapper: a tensor that is not on a HIP device is an error, never a silent host path."""
    for t in tensors:
        if not t.is_cuda:
            raise NativeLibraryError("libtripled_hip needs device tensors (got a %s tensor)" % t.device)


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  The tensor must be a dense CUDA/HIP tensor."""
    if t is None:
        return None
    require_device(t)
    if not t.is_contiguous():
        raise NativeLibraryError("libtripled_hip needs contiguous tensors")
    return ctypes.c_void_p(t.data_ptr())


def ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def stream():
    """torch's current HIP stream as a hipStream_t.  Asked of the runtime directly: every launch asks (native.call), and
    torch.cuda.current_stream() builds a Stream object in Python around the same handle each time."""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


_PLANS = {}      # name -> (arguments in front of the stream, its pointer slots, pointer-array slots, int slots)


def _plan(name):
    slots = SIGNATURES[name][1][:-1]
    where = lambda kind: tuple(i for i, s in enumerate(slots) if s is kind)
    plan = _PLANS[name] = (len(slots), where(_P), where(_PTRARR), where(_I))
    return plan


def call(name, *args, what=None):
    """THE way to launch: ``name`` of SIGNATURES with every argument but the trailing stream, counted by ``check`` as ``what``
    (default: the name).  Pointer slot: None -> NULL, a tensor -> its device pointer, a ready-made c_void_p (a tensor of another
    dense layout whose caller checked it) as it is.  Pointer-array slot: a list / tuple of TENSORS (nothing else) -> a host
    array of their pointers, or a ready-made array.  Every tensor must be on the device (require_device) and dense in planar or
    channels-last order.  int slot: a torch.dtype -> its DTYPE_CODES entry, a bool -> int.  The other slots (floats, long longs,
    host arrays) pass as they are.  A wrong argument count is a TypeError -- ctypes itself lets surplus arguments of a cdecl
    function through.  All of this is checked before the library is loaded or anything is launched.
    (Only the slots that can need work are visited -- the plan is built once per name: an eager step makes ~850 calls.)"""
    arity, pointers, arrays, ints = _PLANS.get(name) or _plan(name)
    if len(args) != arity:
        raise TypeError("%s takes %d arguments in front of the stream, got %d" % (name, arity, len(args)))
    conv = list(args)
    single = [i for i in pointers if conv[i] is not None and type(conv[i]) is not ctypes.c_void_p]
    lists = [i for i in arrays if type(conv[i]) is list or type(conv[i]) is tuple]
    tensors = [conv[i] for i in single]
    for i in lists:
        tensors.extend(conv[i])
    try:
        require_device(*tensors)
        for t in tensors:
            if not (t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)):
                raise NativeLibraryError("libtripled_hip needs contiguous tensors")
    except AttributeError:
        raise TypeError("%s: a pointer argument is a tensor, None or a c_void_p; a pointer array a list of tensors" % name) from None
    for i in single:
        conv[i] = conv[i].data_ptr()
    for i in lists:
        conv[i] = (ctypes.c_void_p * len(conv[i]))(*[t.data_ptr() for t in conv[i]])
    for i in ints:
        a = conv[i]
        if type(a) is not int:
            conv[i] = DTYPE_CODES[a] if type(a) is torch.dtype else int(a)
    conv.append(stream())
    check(getattr(load(), name)(*conv), what or name)


def strides_array(t):
    """Element strides of a 4-D tensor as a host long-long array."""
    return (ctypes.c_longlong * 4)(*[int(v) for v in t.stride()])


def int_array(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])
