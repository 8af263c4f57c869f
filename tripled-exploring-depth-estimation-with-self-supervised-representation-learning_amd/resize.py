"""``Image.resize(size, LANCZOS)`` of uint8 RGB frames, as an exact integer statement (numpy) and on the device (csrc/td_resize.hip).

Replaces, for cfg.data.wire = "raw_u8", ``MonoDataset.resize`` and the flip of ``get_color`` in the loader workers (reference:
mono/datasets/mono_dataset.py:60-63,129-143, ``self.resize = transforms.Resize(..., interpolation=Image.ANTIALIAS)``).  Pillow's
resampler (src/libImaging/Resample.c, precompute_coeffs / normalize_coeffs_8bpc / ImagingResampleHorizontal_8bpc / ..Vertical_8bpc)
is integer arithmetic once the coefficient tables exist, so the device produces the same bytes:

  per axis, in_size -> out_size:  scale = in / out, fs = max(scale, 1), support = 3 fs, ksize = int(ceil(support)) * 2 + 1
  output xx:  center = (xx + 0.5) scale;  xmin = max(int(center - support + 0.5), 0);  xmax = min(int(center + support + 0.5), in) - xmin
              w[x] = L((x + xmin - center + 0.5) * (1 / fs)),  L(t) = sinc(t) sinc(t / 3) on -3 <= t < 3, sinc(t) = sin(pi t) / (pi t)
              w /= sum(w) (summed in order, float64; skipped for a zero sum)
  fixed point:  k = int(w 2^22 + 0.5) (w >= 0), int(w 2^22 - 0.5) (w < 0), both truncating
  a pass:  out = clamp((2^21 + sum_x k[x] pixel[xmin + x]) >> 22, 0, 255) in int32; horizontal first, uint8 in between; a pass
           whose in_size == out_size is skipped.

The flip of the reference happens on the full-size frame, before the resize: ``flip`` makes the horizontal pass read source column
w - 1 - (xmin + x).

The tables depend on the source size only.  ``LanczosBank`` holds them for a list of at most 16 source sizes in ONE device buffer,
built in float64 on the host and uploaded once; ``get_bank`` caches banks per (sizes, out_h, out_w, device).  The per-batch call
``lanczos_resize_hip`` uploads, allocates (beyond its output) and synchronises nothing, so it can be captured into the training
graph; a bank that does not exist yet cannot be built while a stream is capturing (the eager warm-up iterations build it).
"""
import ctypes
import math

import numpy as np
import torch

from . import native

PRECISION_BITS = 22
MAX_SIZES = native.CONSTANTS["TD_RESIZE_MAX_SIZES"]


def _lanczos(t):
    if not (-3.0 <= t < 3.0):
        return 0.0
    if t == 0.0:
        return 1.0
    a, b = t * math.pi, (t / 3.0) * math.pi
    return (math.sin(a) / a) * (math.sin(b) / b)


def lanczos_coeffs(in_size, out_size):
    """(k int32 [out_size, ksize], bounds int32 [out_size, 2] = (xmin, count)): Pillow's 8-bit LANCZOS tables for one axis.  Entries
    of a row beyond its count are 0.  math.sin, not numpy's: the C library's, as Pillow calls it."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError("sizes must be positive, got %d -> %d" % (in_size, out_size))
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    k = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            k[xx, x] = int(v * one - 0.5) if v < 0 else int(v * one + 0.5)
        bounds[xx] = (xmin, xmax)
    return k, bounds


def _pass_numpy(src, k, bounds, axis, reverse=False):
    """One resampling pass over ``axis`` of a uint8 [h, w, c] array; ``reverse`` reads the axis mirrored (the flip)."""
    n_out = k.shape[0]
    shape = list(src.shape)
    shape[axis] = n_out
    out = np.empty(shape, dtype=np.uint8)
    s32 = src.astype(np.int32)
    n_in = src.shape[axis]
    for i in range(n_out):
        lo, cnt = int(bounds[i, 0]), int(bounds[i, 1])
        idx = np.arange(lo, lo + cnt)
        if reverse:
            idx = n_in - 1 - idx
        taps = np.take(s32, idx, axis=axis)
        kk = k[i, :cnt].astype(np.int32)
        kk = kk.reshape([-1 if a == axis else 1 for a in range(src.ndim)])
        acc = (taps * kk).sum(axis=axis, dtype=np.int32) + np.int32(1 << (PRECISION_BITS - 1))
        val = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
        if axis == 0:
            out[i] = val
        else:
            out[:, i] = val
    return out


def lanczos_resize_numpy(img_hwc_u8, out_h, out_w, flip=False):
    """uint8 [h, w, c] -> uint8 [out_h, out_w, c]: the bytes of ``Image.fromarray(img).resize((out_w, out_h), LANCZOS)``, after
    ``transpose(FLIP_LEFT_RIGHT)`` with ``flip``."""
    img = np.asarray(img_hwc_u8)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError("img must be uint8 [h, w, c]")
    h, w = img.shape[:2]
    if w != out_w:
        k, b = lanczos_coeffs(w, out_w)
        img = _pass_numpy(img, k, b, 1, reverse=bool(flip))
    elif flip:
        img = img[:, ::-1]
    if h != out_h:
        k, b = lanczos_coeffs(h, out_h)
        img = _pass_numpy(img, k, b, 0)
    return np.ascontiguousarray(img)


def _axis_tables(in_size, out_size):
    """The tables the kernel applies: a skipped pass (in == out) is the one-tap identity, whose result is the input byte exactly
    ((2^21 + 2^22 p) >> 22 = p)."""
    if in_size == out_size:
        k = np.full((out_size, 1), 1 << PRECISION_BITS, dtype=np.int32)
        b = np.stack([np.arange(out_size), np.ones(out_size)], 1).astype(np.int32)
        return k, b
    return lanczos_coeffs(in_size, out_size)


class LanczosBank:
    """Coefficient tables for the source sizes ``sizes`` [(h, w), ...] -> (out_h, out_w), resident on ``device``.

    tables   int32 device buffer: per size the horizontal coefficients TRANSPOSED [ksx, out_w] (lanes of a wave read consecutive
             columns), horizontal bounds [out_w, 2], vertical coefficients [out_h, ksy], vertical bounds [out_h, 2]
    desc     host int32 [n_sizes, 8]: h, w, ksx, ksy and the four offsets (in ints) into ``tables``
    status   int32 [1] on the device, 0 until a launch meets a size index outside the bank (``bad_index_seen``), tables of other
             sizes, or -- td_lanczos_resize_u8_indexed -- a byte offset outside the resident store
    """

    def __init__(self, sizes, out_h, out_w, device):
        sizes = [(int(h), int(w)) for h, w in sizes]
        if not 1 <= len(sizes) <= MAX_SIZES:
            raise ValueError("a bank holds 1..%d source sizes, got %d" % (MAX_SIZES, len(sizes)))
        if torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("LanczosBank for %r -> %dx%d does not exist yet and cannot be uploaded while the stream is capturing: "
                               "build it (get_bank) in an eager iteration before the capture" % (sizes, out_h, out_w))
        self.sizes, self.out_h, self.out_w = tuple(sizes), int(out_h), int(out_w)
        self.device = torch.device(device)
        parts, desc, off = [], [], 0
        for h, w in sizes:
            kx, bx = _axis_tables(w, self.out_w)
            ky, by = _axis_tables(h, self.out_h)
            for k in (kx, ky):      # the kernel multiplies with the 24-bit integer multiplier
                if int(np.abs(k).max()) >= 1 << 23:
                    raise ValueError("a coefficient of %dx%d -> %dx%d does not fit 24 bits" % (h, w, self.out_h, self.out_w))
            row = [h, w, kx.shape[1], ky.shape[1]]
            for t in (np.ascontiguousarray(kx.T), bx, ky, by):
                row.append(off)
                parts.append(t.reshape(-1))
                off += t.size
            desc.append(row)
        self.desc = np.ascontiguousarray(np.array(desc, dtype=np.int32))
        self.host_tables = np.concatenate(parts).astype(np.int32)
        self.tables = torch.from_numpy(self.host_tables).to(self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.canvas = (max(h for h, _ in sizes), max(w for _, w in sizes))

    def bad_index_seen(self):
        """True if a launch met a size index outside the bank since construction (reads one int back: synchronises)."""
        return bool(int(self.status.item()) != 0)

    def raise_if_bad_index(self):
        """RuntimeError if a launch met a size index outside the bank since the last check; the status word is cleared, so the
        next check reports new launches only.  Synchronises like ``bad_index_seen``."""
        code = int(self.status.item())
        if code == 3:
            self.status.zero_()
            raise RuntimeError("td_lanczos_resize_u8_indexed zero-filled at least one frame: a byte offset outside the resident store for "
                               "the bank of %r -> %dx%d (the loader's 'res_off' and the store on the device disagree)"
                               % (list(self.sizes), self.out_h, self.out_w))
        if code:
            self.status.zero_()
            raise RuntimeError("td_lanczos_resize_u8 zero-filled at least one frame: %s for the bank of %r -> %dx%d (cfg.data.raw_sizes "
                               "and the loader's 'raw_meta' disagree)" % ("a size index outside the bank" if code == 1 else
                               "tables that do not belong to the bank's sizes", list(self.sizes), self.out_h, self.out_w))


_BANKS = {}


def get_bank(sizes, out_h, out_w, device):
    """The cached bank of (sizes, out_h, out_w, device); built and uploaded on first use (not while a stream is capturing)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (tuple((int(h), int(w)) for h, w in sizes), int(out_h), int(out_w), str(device))
    bank = _BANKS.get(key)
    if bank is None:
        bank = _BANKS[key] = LanczosBank(key[0], out_h, out_w, device)
    return bank


def check_banks():
    """``raise_if_bad_index`` of every cached bank.  The per-batch call cannot report a bad device-side size index (it would have
    to synchronise), so the consumers of the 'raw_u8' wire call this where they synchronise anyway: the trainer at the end of an
    epoch, DepthEvaluator after its one copy to the host.  The 'resident' wire's bad byte offsets arrive in the same word and
    are polled here too.  Without a cached bank it does nothing."""
    for bank in list(_BANKS.values()):
        bank.raise_if_bad_index()


def lanczos_resize_hip(frames, meta, bank):
    """frames uint8 [N,3,Hc,Wc] on the bank's device: image n occupies the top-left bank.sizes[meta[n,0]] of its canvas, the rest
    is never read into a result.  meta int32 [N,2] = (size index, flip).  Returns uint8 [N,3,out_h,out_w], bit-equal to
    ``lanczos_resize_numpy`` of each valid region.  One launch on the current stream.

    A ``meta`` on the device is not read by the host (graph capture): an index outside the bank zero-fills that image and raises
    ``bank.status``.  A ``meta`` on the host is checked by the entry point (TD_ERR_BAD_ARG) and uploaded -- the eager / test form."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError("frames must be uint8 [N,3,Hc,Wc]")
    if not frames.is_cuda:
        raise native.NativeLibraryError("lanczos_resize_hip needs device frames (got a %s tensor): there is no host fallback, "
                                        "lanczos_resize_numpy is the test statement" % frames.device)
    if frames.device != bank.device:
        raise ValueError("frames on %s, bank on %s" % (frames.device, bank.device))
    frames = frames.contiguous()
    N, _, Hc, Wc = frames.shape
    if tuple(meta.shape) != (N, 2) or meta.dtype != torch.int32:
        raise ValueError("meta must be int32 [N,2]")
    meta_host = None
    if not meta.is_cuda:
        meta_c = meta.contiguous()
        meta_host = ctypes.cast(meta_c.data_ptr(), ctypes.POINTER(ctypes.c_int))
        meta = meta_c.to(frames.device)
    meta = meta.contiguous()
    out = torch.empty(N, 3, bank.out_h, bank.out_w, dtype=torch.uint8, device=frames.device)
    desc = bank.desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    native.call("td_lanczos_resize_u8", frames, meta, meta_host, bank.tables, int(bank.tables.numel()), desc, len(bank.sizes), N, Hc, Wc,
                bank.out_h, bank.out_w, out, bank.status)
    return out
