"""Host side of the 'raw_u8' wire format (cfg.data.wire = "raw_u8"): decoded frames travel at their NATIVE size, neither flipped nor
resized; both happen on the device, bit-equal to PIL (tripled_amd.resize, csrc/td_resize.hip).

A sample ships
  ("raw_u8", f)  uint8 [3,Hc,Wc]  the frame in the top-left of a fixed canvas (the maximum over cfg.data.raw_sizes), zeros elsewhere:
                                  the stock collate stacks KITTI's mixed sizes
  "raw_meta"     int32 [2]        (index of the frame's (h, w) in cfg.data.raw_sizes, flip); the frames of a sample share it
  "raw_spec"     int32 [2 + 2n]   (H, W, h0, w0, h1, w1, ...): the network size and the size list, i.e. which coefficient bank expands
                                  the batch.  It STAYS ON THE HOST through every staging step (HOST_KEYS), so the expansion reads it
                                  without a device synchronisation, inside a captured graph too.  It repeats the dataset's
                                  configuration per sample so that a batch describes itself; the expansion requires all rows of a
                                  batch to be equal, and a captured graph keeps the bank of the batch it was captured on
  "aug"          float [9]        as the 'uint8' wire

The 'resident' wire (cfg.data.wire = "resident", tripled_amd.resident) ships, instead of the canvases,
  ("res_off", f) int64 []         the byte offset of the frame in the store resident on the device; int64 through every staging step
  "res_bytes"    int64 [1]        the store's length by the index the dataset read: a HOST key like "raw_spec"; the expansion compares it
                                  with the store loaded on the device
and "raw_meta", "raw_spec", "aug" unchanged.
"""
import numpy as np
import torch

KITTI_RAW_SIZES = ((375, 1242), (370, 1224), (370, 1226), (374, 1238), (376, 1241))
BYTE_FRAMES = ("color_u8", "raw_u8")     # tuple keys whose tensors stay uint8 until the device-side expansion
HOST_KEYS = ("raw_spec", "res_bytes")    # entries that are never moved to the device
OFFSET_FRAMES = ("res_off",)             # tuple keys whose tensors stay int64: byte offsets into the resident store ('resident' wire)


def is_byte_frame(key):
    return isinstance(key, tuple) and bool(key) and key[0] in BYTE_FRAMES


def keeps_dtype(key):
    """Entries every staging step moves to the device as they are -- bytes, int32 "raw_meta", int64 offsets (a float32 cast would
    lose the bits of an offset above 2^24) -- until the device-side expansion consumes them."""
    return key == "raw_meta" or is_byte_frame(key) or (isinstance(key, tuple) and bool(key) and key[0] in OFFSET_FRAMES)


def raw_sizes_of(cfg):
    sizes = cfg.get("raw_sizes", None) if cfg is not None else None
    sizes = KITTI_RAW_SIZES if sizes is None else sizes
    sizes = tuple((int(h), int(w)) for h, w in sizes)
    if not 1 <= len(sizes) <= 16:
        raise ValueError("cfg.data.raw_sizes must list 1..16 (h, w) sizes, got %d" % len(sizes))
    return sizes


def canvas_of(sizes):
    return max(h for h, _ in sizes), max(w for _, w in sizes)


def raw_spec(height, width, sizes):
    return torch.tensor([int(height), int(width)] + [int(v) for s in sizes for v in s], dtype=torch.int32)


def parse_spec(spec_row):
    """One row of a collated "raw_spec" -> (H, W, sizes)."""
    v = [int(x) for x in spec_row.tolist()]
    return v[0], v[1], tuple(zip(v[2::2], v[3::2]))


def size_index(h, w, sizes):
    try:
        return sizes.index((int(h), int(w)))
    except ValueError:
        raise ValueError("a frame of %dx%d (h x w) is not in cfg.data.raw_sizes = %r: the 'raw_u8' wire resizes on the device with "
                         "tables built for the listed sizes only -- add the size to cfg.data.raw_sizes" % (h, w, list(sizes))) from None


def to_canvas(frame_chw_u8, canvas):
    """uint8 [3,h,w] (tensor or array) -> uint8 [3,Hc,Wc] with the frame in the top-left corner."""
    frame = torch.as_tensor(np.ascontiguousarray(frame_chw_u8)) if not torch.is_tensor(frame_chw_u8) else frame_chw_u8
    out = torch.zeros(3, canvas[0], canvas[1], dtype=torch.uint8)
    out[:, :frame.shape[1], :frame.shape[2]] = frame
    return out
