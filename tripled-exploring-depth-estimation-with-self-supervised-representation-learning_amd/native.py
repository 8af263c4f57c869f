"""ctypes binding of libtripled_hip.so (C ABI: include/tripled_hip.h).

There is deliberately no fallback: if the shared library is missing or a call returns an
error code, an exception is raised.  Nothing in here touches ``oracle/``.
"""
import ctypes
import os

import torch

from . import dispatch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtripled_hip.so")

TD_MAX_SRC = 4

# name -> (restype, argtypes); mirrors include/tripled_hip.h one to one
_PTRARR = ctypes.POINTER(ctypes.c_void_p)
_I, _F, _P = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
_LLARR = ctypes.POINTER(ctypes.c_longlong)     # host arrays
_IARR = ctypes.POINTER(ctypes.c_int)
ABI_VERSION = 3      # include/tripled_hip.h: TD_ABI_VERSION

SIGNATURES = {
    "td_abi_version": (_I, []),
    "td_error_string": (ctypes.c_char_p, [_I]),
    "td_last_hip_error": (ctypes.c_char_p, []),
    "td_photo_num_blocks": (_I, [_I, _I, _I]),
    "td_photo_bwd_num_blocks": (_I, [_I, _I, _I]),
    "td_photo_identity": (_I, [_P, _PTRARR, _I, _I, _I, _I, _P, _P, _PTRARR, _P]),
    "td_photo_fwd": (_I, [_P, _PTRARR, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P]),
    "td_photo_bwd": (_I, [_P, _PTRARR, _P, _PTRARR, _I, _P, _P, _P, _P, _P, _I, _P, _F, _I, _I, _I, _I, _I, _F, _F, _P, _P, _P]),
    "td_pack_rgbx": (_I, [_P, _I, _I, _I, _P, _P]),
    "td_upsample_adjoint": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, _P]),
    "td_upsample_adjoint_planes": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "td_reduce_dP": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "td_sum_scaled": (_I, [_P, _I, _F, _P, _P]),
    "td_area_downsample": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "td_smooth_num_blocks": (_I, [_I, _I, _I]),
    "td_smooth_fwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "td_smooth_finish": (_I, [_P, _I, _I, _I, _F, _P, _P]),
    "td_smooth_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _F, _P, _P, _P, _I, _P]),
    "td_maxpool5_fwd": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "td_maxpool5_bwd": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "td_maxpool5_bwd_add": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "td_conv1x1_fwd_sum": (_I, [_P, _P, ctypes.c_longlong, _I, _I, _P, _P, _P, _P]),
    "td_maxpool3s2_fwd": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "td_maxpool3s2_bwd": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "td_join_fwd": (_I, [_P, _P, _P, _I, ctypes.c_longlong, _I, _I, _I, _P, _P]),
    "td_join_bwd": (_I, [_P, _I, ctypes.c_longlong, _I, _I, _I, _P, _P, _P, _P]),
    "td_join_up2_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "td_join_up2_bwd": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "td_bn_workspace_floats": (ctypes.c_longlong, [ctypes.c_longlong, _I, _I]),
    "td_bn_fwd": (_I, [_P, _P, _I, _P, _P, _P, _P, _F, _F, _I, ctypes.c_longlong, _I, _I, _P, _P, _P, _P, _P]),
    "td_conv1x1_stat_rows": (_I, [ctypes.c_longlong, _I, _I]),
    "td_conv1x1_fwd": (_I, [_P, _P, ctypes.c_longlong, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "td_conv3x3_fwd": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "td_conv3x3_wgrad_workspace_floats": (ctypes.c_longlong, [_I, _I, _I, _I, _I]),
    "td_conv3x3_wgrad": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "td_conv1x1_wgrad_workspace_floats": (ctypes.c_longlong, [ctypes.c_longlong, _I, _I]),
    "td_conv1x1_wgrad": (_I, [_P, _P, ctypes.c_longlong, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "td_conv1x1_wgrad_group": (_I, [_I, _PTRARR, _PTRARR, _LLARR, _IARR, _IARR, _IARR, _IARR, _IARR, _IARR, _PTRARR, _PTRARR, _P]),
    "td_bn_fwd_from_partials": (_I, [_P, _P, _I, _P, _P, _P, _P, _F, _F, _I, ctypes.c_longlong, _I, _I, _P, _I, _P, _P, _P, _P]),
    "td_bias_act_workspace_floats": (ctypes.c_longlong, [ctypes.c_longlong, _I]),
    "td_bias_act_fwd": (_I, [_P, _P, _I, _I, ctypes.c_longlong, _I, _I, _P, _P]),
    "td_bias_act_bwd": (_I, [_P, _P, _I, ctypes.c_longlong, _I, _I, _P, _P, _I, _P, _P]),
    "td_gather_flat": (_I, [_PTRARR, _LLARR, _LLARR, _I, _I, _P, _P]),
    "td_adam_flat": (_I, [_P, _P, _P, _P, _P, ctypes.c_longlong, ctypes.c_longlong, _P, _P, _F, ctypes.c_double, ctypes.c_double, _F, _P, _F, _P]),
    "td_bn_partial_rows": (_I, [ctypes.c_longlong, _I, _I]),
    "td_bn_fwd_partials": (_I, [_P, _I, ctypes.c_longlong, _I, _I, _P, _P]),
    "td_bn_bwd_partials": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _I, ctypes.c_longlong, _I, _I, _P, _P]),
    "td_bn_bwd_from_partials": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _I, ctypes.c_longlong, _I, _I, _P, _I, _P, _P, _P, _P, _P]),
    "td_conv1x1_fwd_bnrelu": (_I, [_P, _P, ctypes.c_longlong, _I, _I, _I, _P, _I, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P]),
    "td_conv1x1_dgrad": (_I, [_P, _P, ctypes.c_longlong, _I, _I, _I, _P, _P, _P]),
    "td_conv1x1_dgrad_bnsums": (_I, [_P, _P, ctypes.c_longlong, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "td_conv1x1_dgrad_bnbwd": (_I, [_P, _P, _P, ctypes.c_longlong, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "td_bn_bwd": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _I, ctypes.c_longlong, _I, _I, _P, _P, _P, _P, _P, _P]),
    "td_edge_weights": (_I, [_P, _I, _I, _I, _F, ctypes.POINTER(ctypes.c_float), _P, _P]),
    "td_featreg_num_blocks": (_I, [_I, _I, _I, _I]),
    "td_featreg_fwd": (_I, [_P, _I, _P, _I, _I, _I, _I, _P, _P]),
    "td_featreg_bwd": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _P, _P]),
    "td_recon_num_tasks": (_I, [_I, _I, _I]),
    "td_recon_fwd": (_I, [_P, _P, _P, _I, _I, _I, _P, _P]),
    "td_recon_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "td_reflpad1_fwd": (_I, [_P, _I, _I, _I, _I, _I, _P, _P]),
    "td_reflpad1_bwd": (_I, [_P, _I, _I, _I, _I, _I, _P, _P]),
    "td_up2_reflpad1_fwd": (_I, [_P, _I, _I, _I, _I, _I, _P, _P]),
    "td_up2_reflpad1_bwd": (_I, [_P, _I, _I, _I, _I, _I, _P, _P]),
    "td_featwarp_num_blocks": (_I, [_I, _I, _I]),
    "td_featwarp_fwd": (_I, [_P, _PTRARR, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _F, _P, _P, _P]),
    "td_featwarp_bwd": (_I, [_P, _PTRARR, _I, _I, _P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _I, _I, _F, _F, _P, _PTRARR,
                             _P, _P, _P]),
    "td_featwarp_dsrc_finish": (_I, [_P, _P, _F, _I, ctypes.c_longlong, _I, _P, _P]),
    "td_reduce_partials": (_I, [_P, _I, _I, _I, _P, _P]),
    "td_bn_sync_fwd_sums": (_I, [_P, _I, ctypes.c_longlong, _I, _I, _P, _P, _P]),
    "td_bn_sync_fwd_apply": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _F, _F, _I, ctypes.c_longlong, _I, _I, _P, _P, _P, _P]),
    "td_bn_sync_bwd_sums": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _I, ctypes.c_longlong, _I, _I, _P, _P, _P]),
    "td_bn_sync_bwd_dx": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, ctypes.c_longlong, _I, _I, _P, _P, _P, _P, _P, _P]),
    "td_fp8_num_blocks": (_I, [ctypes.c_longlong]),
    "td_fp8_amax_partials": (_I, [_P, _I, ctypes.c_longlong, _P, _P]),
    "td_fp8_quantize": (_I, [_P, _I, ctypes.c_longlong, _P, _P, _P, _P]),
    "td_color_jitter": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "td_l1map_fwd": (_I, [_P, _I, _LLARR, _P, _I, _I, _I, _I, _F, _P, _P]),
    "td_l1map_bwd": (_I, [_P, _I, _LLARR, _P, _P, _I, _I, _I, _I, _F, _P, _P]),
    "td_rgb2lab": (_I, [_P, _I, _I, _I, _F, _F, _F, _P, _P]),
    "td_pose_fwd": (_I, [_P, _P, _IARR, _P, _I, _I, _P, _P, _P]),
    "td_pose_bwd": (_I, [_P, _P, _IARR, _P, _I, _I, _P, _P, _P, _P, _P]),
    "td_infer_preprocess": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "td_disp_postprocess": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _F, _F, _F, _P, _P, _P]),
    "td_colorize": (_I, [_P, _I, ctypes.c_longlong, _P, _P, _P, _P, _P]),
    "td_eval_depth_workspace_bytes": (ctypes.c_longlong, [_I, _I, _I]),
    "td_eval_depth": (_I, [_P, _I, _I, _I, _I, _F, _F, _P, _I, _I, _P, _P, _F, _F, _I, _P, ctypes.c_longlong, _P, _P, _P]),
    "td_masked_median_workspace_bytes": (ctypes.c_longlong, [_I]),
    "td_masked_median": (_I, [_P, _I, ctypes.c_longlong, _P, ctypes.c_longlong, _P, _P, _P]),
    "td_pose_pairs_u8": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, ctypes.c_longlong, _P]),
    "td_odom_trajectory": (_I, [_P, _I, _I, _P, _P]),
    "td_odom_snippet_ate": (_I, [_P, _I, _P, _I, _I, _P, _P]),
    "td_odom_sequence_errors": (_I, [_P, _P, _I, ctypes.POINTER(ctypes.c_double), _I, _I, _I, _P, _P, _P, _P, _P]),
    "td_lanczos_resize_u8": (_I, [_P, _P, _IARR, _P, ctypes.c_longlong, _IARR, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "td_lanczos_resize_u8_indexed": (_I, [_P, ctypes.c_longlong, _P, _LLARR, _P, _IARR, _P, ctypes.c_longlong, _IARR, _I, _I, _I, _I, _P,
                                          _P, _P]),
    "td_cloud_keys": (_I, [_P, _P, _P, ctypes.POINTER(ctypes.c_double), _I, _I, _I, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                           _I, _I, ctypes.c_double, ctypes.c_double, _F, _P, _P, _P, _P]),
    "td_cloud_heads": (_I, [_P, ctypes.c_longlong, _P, _P]),
    "td_cloud_reduce_packed": (_I, [_P, _P, _P, _P, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, _P, _P, _P]),
    "td_cloud_reduce_rows": (_I, [_P, _P, _P, _P, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, _P, _P, _P]),
    "td_cloud_finish": (_I, [_P, _P, ctypes.c_longlong, ctypes.c_double, ctypes.c_longlong, _P, _P, _P, _P, _P]),
    "td_cloud_views": (_I, [_P, _P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), _I, _I, _I, _I, _I, _I, _I, _I, _I,
                            ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _P, _P, _P, _P, _P]),
    "td_velo_depth_workspace_bytes": (ctypes.c_longlong, [_I, _I, _I]),
    "td_velo_depth": (_I, [_P, _P, _I, _P, _P, _I, _I, _I, _P, ctypes.c_longlong, _P, _P, _P]),
    "td_cloud_render_workspace_bytes": (ctypes.c_longlong, [_I, _I, _I]),
    "td_cloud_render": (_I, [_P, _P, ctypes.c_longlong, _P, ctypes.POINTER(ctypes.c_double), _I, _I, _I, ctypes.c_double, ctypes.c_double,
                             ctypes.c_double, ctypes.c_double, _I, _I, _I, _I, _P, ctypes.c_longlong, _P, _P, _P, _P, _P]),
    "td_scan_keys": (_I, [_P, ctypes.c_longlong, _P, _I, ctypes.POINTER(ctypes.c_double), _P, ctypes.POINTER(ctypes.c_double), _I, _I,
                          ctypes.c_double, ctypes.c_double, ctypes.c_double, _P, _P, _P, _P]),
    "td_nn_query": (_I, [_P, ctypes.c_longlong, _P, _P, ctypes.c_longlong, _P, _P, ctypes.c_longlong, ctypes.c_double,
                         ctypes.POINTER(ctypes.c_double), _I, _P, _P, _P, _P]),
    "td_cloud_transform": (_I, [_P, ctypes.c_longlong, ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                _P, _P]),
    "td_icp_moments_workspace": (ctypes.c_longlong, [ctypes.c_longlong]),
    "td_icp_moments": (_I, [_P, ctypes.c_longlong, _P, ctypes.c_longlong, _P, _P, ctypes.c_double, ctypes.POINTER(ctypes.c_double), _P,
                            ctypes.c_longlong, _P, _P]),
    "td_cloud_normals": (_I, [_P, ctypes.c_longlong, _P, ctypes.c_longlong, _P, _P, ctypes.c_longlong, ctypes.c_double, ctypes.c_double,
                              ctypes.c_double, ctypes.c_longlong, ctypes.c_double, _P, _P, _P, _P, _P]),
    "td_icp_plane_moments_workspace": (ctypes.c_longlong, [ctypes.c_longlong]),
    "td_icp_plane_moments": (_I, [_P, ctypes.c_longlong, _P, _P, ctypes.c_longlong, _P, _P, ctypes.c_double,
                                  ctypes.POINTER(ctypes.c_double), _P, ctypes.c_longlong, _P, _P]),
    "td_normals_orient": (_I, [_P, _P, ctypes.c_longlong, _P, _I, ctypes.c_double, _P, _P, _P, _P]),
    "td_cloud_render_surfels": (_I, [_P, _P, _P, ctypes.c_longlong, _P, ctypes.POINTER(ctypes.c_double), _I, _I, _I, ctypes.c_double,
                                     ctypes.c_double, ctypes.c_double, ctypes.c_double, _I, _I, ctypes.c_double, _I, _I, _I, _I, _P,
                                     ctypes.c_longlong, _P, _P, _P, _P, _P, _P]),
}

DTYPE_CODES = {torch.float32: 0, torch.bfloat16: 1}


class NativeLibraryError(RuntimeError):
    pass


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
        hip = lib.td_last_hip_error().decode()
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
