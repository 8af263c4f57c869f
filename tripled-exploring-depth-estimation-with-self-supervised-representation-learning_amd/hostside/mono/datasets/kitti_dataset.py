"""KITTI raw frame-triplet datasets (reference: mono/datasets/mono_dataset.py:40-201,
mono/datasets/kitti_dataset.py:121-202), written without torchvision: PIL does the decoding, the
LANCZOS resize (the reference's Image.ANTIALIAS) and the colour jitter (the same PIL ImageEnhance /
HSV-shift primitives torchvision's ColorJitter applies to PIL images, in a random order).

Sample contract (what the models consume): ("color", f, 0) and ("color_aug", f, 0) float [3,H,W] in
[0,1] for every f in frame_idxs, "K" / "inv_K" [4,4] (normalised intrinsics scaled by W, H; inv_K =
pinv(K)), ("mask", 0, 0) uint8 [3,H,W] for the in-painting variant, "stereo_T" when 's' is a frame id,
"gt_depth" in validation.  Split lists are plain text: "<folder> <frame_index> <l|r>" per line.

Ground truth of a validation sample (cfg.data.gt_source): "archive" (default) serves "gt_depth" from gt_depth_path, an .npz whose
"data" is either one [n,H,W] array or, with a "sizes" int32 [n,2] entry next to it, zero-padded maps of different sizes
(tools/export_gt_depth.py); "velodyne" ships the frame's raw scan instead -- "velo" float32 [N,4], "velo_P" float64 [3,4], "gt_size"
int32 [2] -- and the evaluation makes the map (tripled_amd.velodyne; KITTIRAWDataset.get_depth is the same map on the host).
"""
import os
import random

import numpy as np
import torch
from PIL import Image, ImageEnhance
from torch.utils.data import Dataset

from . import raw_wire as raw_wire_mod

LANCZOS = getattr(Image, "Resampling", Image).LANCZOS
FLIP = getattr(Image, "Transpose", Image).FLIP_LEFT_RIGHT


def read_split(split, which, split_dir=None):
    """Lines of <split_dir>/<split>/<which>_files.txt (default: mono/datasets/splits next to this file)."""
    root = split_dir or os.path.join(os.path.dirname(__file__), "splits")
    path = os.path.join(root, split, "{}_files.txt".format(which))
    with open(path) as f:
        return f.read().splitlines()


def pil_loader(path):
    with open(path, "rb") as f:
        with Image.open(f) as img:
            return img.convert("RGB")


def to_tensor(img):
    """PIL RGB -> float [3,H,W] in [0,1] (torchvision ToTensor semantics)."""
    return to_uint8(img).float().div_(255.0)


def to_uint8(img):
    """PIL RGB -> uint8 [3,H,W] (the 'uint8' wire format: 3 bytes per pixel instead of 2 x 12)."""
    arr = np.array(img, dtype=np.uint8)
    return torch.from_numpy(arr).permute(2, 0, 1).contiguous()


def _shift_hue(img, hue_factor):
    h, s, v = img.convert("HSV").split()
    arr = np.asarray(h, dtype=np.uint8).astype(np.int16)
    arr = ((arr + int(hue_factor * 255)) % 256).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(arr, "L"), s, v)).convert("RGB")


class ColorJitter:
    """One draw of (order, brightness, contrast, saturation, hue), applied identically to every image it is
    called on -- the reference's stated intent for the frames of one sample (mono_dataset.py:89-95)."""

    def __init__(self, brightness, contrast, saturation, hue):
        self.order = torch.randperm(4).tolist()
        self.factors = [float(torch.empty(1).uniform_(*brightness)), float(torch.empty(1).uniform_(*contrast)),
                        float(torch.empty(1).uniform_(*saturation)), float(torch.empty(1).uniform_(*hue))]

    def as_row(self):
        """(enabled, op0..op3, brightness, contrast, saturation, hue): the parameter row td_color_jitter consumes."""
        return torch.tensor([1.0] + [float(o) for o in self.order] + self.factors, dtype=torch.float32)

    def __call__(self, img):
        for op in self.order:
            if op == 0:
                img = ImageEnhance.Brightness(img).enhance(self.factors[0])
            elif op == 1:
                img = ImageEnhance.Contrast(img).enhance(self.factors[1])
            elif op == 2:
                img = ImageEnhance.Color(img).enhance(self.factors[2])
            else:
                img = _shift_hue(img, self.factors[3])
        return img


class MonoDataset(Dataset):
    brightness, contrast, saturation, hue = (0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1)

    def __init__(self, data_path, filenames, height, width, frame_idxs, cfg=None, is_train=False, img_ext=".jpg",
                 gt_depth_path=None):
        super().__init__()
        self.data_path, self.filenames = data_path, filenames
        self.height, self.width = height, width
        self.frame_idxs, self.is_train, self.img_ext = list(frame_idxs), is_train, img_ext
        self.cfg = cfg if cfg is not None else {}
        self.loader = pil_loader
        self.gt_depth_path = gt_depth_path
        self.flag = np.zeros(len(self), dtype=np.int64)        # single aspect-ratio group for the samplers
        self.gt_depths = None
        self.gt_sizes = None
        self._raw = None
        self._store_index = None
        if not is_train and gt_depth_path is not None and os.path.exists(str(gt_depth_path)):
            # the reference loads this archive with allow_pickle=True; object arrays are refused here
            archive = np.load(gt_depth_path, allow_pickle=False)
            self.gt_depths = archive["data"]
            if "sizes" in archive.files:      # maps of different sizes, zero-padded to the largest (tools/export_gt_depth.py)
                self.gt_sizes = np.asarray(archive["sizes"], dtype=np.int64).reshape(-1, 2)
                if self.gt_depths.ndim != 3 or len(self.gt_sizes) != len(self.gt_depths):
                    raise ValueError("%s: 'sizes' [n,2] next to 'data' [n,Hmax,Wmax], got %s and %s"
                                     % (gt_depth_path, self.gt_sizes.shape, self.gt_depths.shape))

    def __len__(self):
        return len(self.filenames)

    def resize(self, img):
        return img.resize((self.width, self.height), LANCZOS)

    def get_color(self, folder, frame_index, side, do_flip):
        raise NotImplementedError

    def get_velodyne(self, folder, frame_index, side):
        raise NotImplementedError("cfg.data.gt_source = 'velodyne' needs a dataset with raw scans (KITTIRAWDataset)")

    def _raw_layout(self):
        """(sizes, canvas, "raw_spec") of the 'raw_u8' wire format: fixed by the configuration, worked out once."""
        if self._raw is None:
            sizes = raw_wire_mod.raw_sizes_of(self.cfg)
            self._raw = (sizes, raw_wire_mod.canvas_of(sizes), raw_wire_mod.raw_spec(self.height, self.width, sizes))
        return self._raw

    def _resident_index(self):
        """The index of cfg.data.store ('resident' wire), read once per process and checked against this dataset's configuration."""
        if self._store_index is None:
            from tripled_amd import resident
            store = self.cfg.get("store", None)
            if not store:
                raise ValueError("cfg.data.wire = 'resident' needs cfg.data.store, the directory tools/pack_frames.py wrote")
            index = resident.load_index(store)
            index.check_config(self.img_ext, self._raw_layout()[0])
            self._store_index = index
        return self._store_index

    def _resident_frame(self, index, folder, frame_index, side):
        """(byte offset, h, w) of a frame in the store, or None when the packer did not find the file."""
        from tripled_amd import resident
        return index.frames.get(resident.relative_path(self, folder, frame_index, side))

    def postprocess(self, inputs):
        """Hook for subclasses (in-painting masks)."""

    def frame_u8(self, index, offset=0):
        """The frame ``offset`` after the one line ``index`` names, decoded once and resized like a sample's frames: uint8
        [3,H,W], no augmentation.  A consumer that needs every frame of a sequence (tripled_amd.odometry) reads n+1 frames this way
        instead of n samples of two frames each."""
        parts = self.filenames[index].split()
        frame_index = int(parts[1]) if len(parts) == 3 else 0
        side = parts[2] if len(parts) == 3 else None
        return to_uint8(self.resize(self.get_color(parts[0], frame_index + offset, side, False)))

    def __getitem__(self, index):
        inputs = {}
        do_color_aug = self.is_train and random.random() > 0.5
        do_flip = self.is_train and random.random() > 0.5
        parts = self.filenames[index].split()
        folder = parts[0]
        frame_index = int(parts[1]) if len(parts) == 3 else 0
        side = parts[2] if len(parts) == 3 else None
        if not self.is_train and self.cfg.get("gt_source", "archive") == "velodyne":
            inputs.update(self.get_velodyne(folder, frame_index, side))
        elif self.gt_depths is not None and self.gt_sizes is not None:
            h, w = self.gt_sizes[index]
            inputs["gt_depth"] = self.gt_depths[index, :h, :w]
        elif self.gt_depths is not None:
            inputs["gt_depth"] = self.gt_depths[index]
        jitter = ColorJitter(self.brightness, self.contrast, self.saturation, self.hue) if do_color_aug else None
        # wire = "uint8": frames travel as bytes, ToTensor and the colour jitter run on the device
        # (mono.datasets.device_expand / csrc/td_augment.hip); "float32" is the reference's format
        # wire = "raw_u8": the frames travel at their native size; the flip and the LANCZOS resize run on the device too
        # (mono.datasets.raw_wire / csrc/td_resize.hip), with the same draws in the same order
        wire = self.cfg.get("wire", "float32")
        # wire = "resident": as "raw_u8", but the decoded frames already live in device memory (tripled_amd.resident): no file is
        # opened, a frame travels as its byte offset in the store
        res_wire = wire == "resident"
        raw_wire = wire == "raw_u8" or res_wire
        u8_wire = wire == "uint8" or raw_wire
        if u8_wire:
            inputs["aug"] = jitter.as_row() if jitter is not None else torch.zeros(9)
        load_flipped = do_flip and not raw_wire
        raw_index = None
        sizes, canvas, spec = self._raw_layout() if raw_wire else (None, None, None)
        store_index = self._resident_index() if res_wire else None
        for i in self.frame_idxs:
            if res_wire:
                other = {"r": "l", "l": "r"}[side] if i == "s" else side
                entry = self._resident_frame(store_index, folder, frame_index + (0 if i == "s" else i), other)
                if entry is None and i != "s":                   # sequence boundary: repeat the centre frame
                    entry = self._resident_frame(store_index, folder, frame_index, side)
                if entry is None:
                    raise ValueError("%s does not list %s (sample %d): pack the store from the split lists this dataset reads"
                                     % (store_index.path, self.get_image_path(folder, frame_index, other), index))
                idx = raw_wire_mod.size_index(entry[1], entry[2], sizes)
                if raw_index is not None and idx != raw_index:
                    raise ValueError("the frames of sample %d have different sizes in %s: 'raw_meta' is one size index per sample"
                                     % (index, store_index.path))
                raw_index = idx
                inputs[("res_off", i)] = torch.tensor(entry[0], dtype=torch.int64)
                continue
            if i == "s":
                img = self.get_color(folder, frame_index, {"r": "l", "l": "r"}[side], load_flipped)
            else:
                try:
                    img = self.get_color(folder, frame_index + i, side, load_flipped)
                except (FileNotFoundError, OSError):            # sequence boundary: repeat the centre frame
                    img = self.get_color(folder, frame_index, side, load_flipped)
            if raw_wire:
                idx = raw_wire_mod.size_index(img.height, img.width, sizes)
                if raw_index is not None and idx != raw_index:
                    raise ValueError("the frames of sample %d have different sizes: 'raw_meta' is one size index per sample" % index)
                raw_index = idx
                inputs[("raw_u8", i)] = raw_wire_mod.to_canvas(to_uint8(img), canvas)
                continue
            img = self.resize(img)
            if u8_wire:
                inputs[("color_u8", i)] = to_uint8(img)
                continue
            inputs[("color", i, 0)] = to_tensor(img)
            inputs[("color_aug", i, 0)] = to_tensor(jitter(img)) if jitter is not None else inputs[("color", i, 0)].clone()
        if raw_wire:
            inputs["raw_meta"] = torch.tensor([raw_index, int(do_flip)], dtype=torch.int32)
            inputs["raw_spec"] = spec.clone()
        if res_wire:
            inputs["res_bytes"] = torch.tensor([store_index.total_bytes], dtype=torch.int64)
        K = self.K.copy()
        K[0, :] *= self.width
        K[1, :] *= self.height
        inputs["K"] = torch.from_numpy(K)
        inputs["inv_K"] = torch.from_numpy(np.linalg.pinv(K))
        self.postprocess(inputs)
        if "s" in self.frame_idxs:
            stereo_T = np.eye(4, dtype=np.float32)
            stereo_T[0, 3] = (-1 if side == "l" else 1) * (-1 if do_flip else 1) * 0.015
            inputs["stereo_T"] = torch.from_numpy(stereo_T)
        return inputs


class KITTIDataset(MonoDataset):
    K = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    full_res_shape = (1242, 375)
    side_map = {"2": 2, "3": 3, "l": 2, "r": 3}

    def get_image_path(self, folder, frame_index, side):
        name = "{:010d}{}".format(frame_index, self.img_ext)
        return os.path.join(self.data_path, folder, "image_0{}/data".format(self.side_map[side]), name)

    def get_color(self, folder, frame_index, side, do_flip):
        img = self.loader(self.get_image_path(folder, frame_index, side))
        return img.transpose(FLIP) if do_flip else img

    def check_depth(self):
        parts = self.filenames[0].split()
        velo = os.path.join(self.data_path, parts[0], "velodyne_points/data/{:010d}.bin".format(int(parts[1])))
        return os.path.isfile(velo)


class KITTIRAWDataset(KITTIDataset):
    """KITTI raw with ground truth from the velodyne scans (reference kitti_dataset.py:189-215)."""

    def _calibration(self, folder, side):
        """(P, (H, W)) of the folder's date and the side's camera, read once per process."""
        from tripled_amd import velodyne
        cache = self.__dict__.setdefault("_velo_calib", {})
        key = (folder.split("/")[0], self.side_map[side])
        if key not in cache:
            cache[key] = velodyne.velo_to_image(os.path.join(self.data_path, key[0]), key[1])
        return cache[key]

    def get_velodyne_path(self, folder, frame_index):
        return os.path.join(self.data_path, folder, "velodyne_points/data/{:010d}.bin".format(int(frame_index)))

    def get_velodyne(self, folder, frame_index, side):
        """The three keys of a validation sample under gt_source = 'velodyne'."""
        from tripled_amd import velodyne
        P, size = self._calibration(folder, side)
        return {"velo": torch.from_numpy(velodyne.load_velodyne_points(self.get_velodyne_path(folder, frame_index))),
                "velo_P": torch.from_numpy(P.copy()), "gt_size": torch.tensor(size, dtype=torch.int32)}

    def get_depth(self, folder, frame_index, side, do_flip):
        """The reference's method on the host statement: the map at native size, float32, mirrored when flipped.  The reference's
        scipy.misc.imresize to full_res_shape is left out (it byte-scaled the map; the evaluation reads native size)."""
        from tripled_amd import velodyne
        P, (h, w) = self._calibration(folder, side)
        points = velodyne.load_velodyne_points(self.get_velodyne_path(folder, frame_index))
        depth_gt = velodyne.depth_map_numpy(points, P, h, w)[0].astype(np.float32)
        return np.fliplr(depth_gt) if do_flip else depth_gt


class KITTIInpaintDataset(KITTIDataset):
    """Adds ("mask", 0, 0): ones with `erase_count` zeroed `erase_shape` rectangles (one centred square when
    erase_count == 1), reference kitti_dataset.py:167-182."""

    def postprocess(self, inputs):
        if ("raw_u8", 0) in inputs or ("res_off", 0) in inputs:     # 'raw_u8' / 'resident' wire: no frame of the network size yet
            shape = (3, self.height, self.width)
        else:
            shape = tuple((inputs[("color", 0, 0)] if ("color", 0, 0) in inputs else inputs[("color_u8", 0)]).shape)
        eh, ew = self.cfg["erase_shape"]
        count = self.cfg["erase_count"]
        mask = torch.ones(shape, dtype=torch.uint8)
        if count == 1:
            off = int((shape[1] - eh) / 2)
            mask[:, off:off + eh, off:off + eh] = 0
        else:
            for _ in range(count):
                row = int(torch.randint(0, shape[1] - eh - 1, (1,)))
                col = int(torch.randint(0, shape[2] - ew - 1, (1,)))
                mask[:, row:row + eh, col:col + ew] = 0
        inputs[("mask", 0, 0)] = mask


class KITTIOdomDataset(KITTIDataset):
    """KITTI odometry sequences (reference kitti_dataset.py:324-338): <data_path>/sequences/<NN>/image_<0|1>/<%06d><ext>; the
    folder field of a line is the sequence number."""
    side_map = {"l": 0, "r": 1}

    def get_image_path(self, folder, frame_index, side):
        name = "{:06d}{}".format(frame_index, self.img_ext)
        return os.path.join(self.data_path, "sequences/{:02d}".format(int(folder)), "image_{}".format(self.side_map[side]), name)


def odom_sequence_files(seq, n_frames):
    """The lines "<seq> <i> l" for i in 0 ... n_frames-2: one per consecutive frame pair of a sequence of n_frames frames (the
    contents of the reference's splits/odom/test_files_09.txt / _10.txt for n_frames = 1591 / 1201)."""
    if int(n_frames) < 2:
        raise ValueError("a sequence needs at least two frames, got %r" % (n_frames,))
    return ["{} {} l".format(int(seq), i) for i in range(int(n_frames) - 1)]
