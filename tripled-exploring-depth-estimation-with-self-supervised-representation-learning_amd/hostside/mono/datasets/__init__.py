from .loader import DistributedGroupSampler, DistributedSampler, GroupSampler, build_dataloader  # noqa: F401
from .get_dataset import get_dataset  # noqa: F401
from .synthetic import ResidentBatches, SyntheticTripletDataset, synthetic_batch  # noqa: F401
from .prefetch import DevicePrefetcher  # noqa: F401
from .device_expand import collate_validation, expand_device_batch, has_uint8_frames  # noqa: F401


def __getattr__(name):      # the KITTI classes need PIL: imported on first use
    if name in ("KITTIOdomDataset", "KITTIRAWDataset", "KITTIInpaintDataset", "odom_sequence_files"):
        from . import kitti_dataset
        return getattr(kitti_dataset, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
