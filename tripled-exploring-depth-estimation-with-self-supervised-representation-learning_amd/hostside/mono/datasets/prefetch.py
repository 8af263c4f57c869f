"""Host->device input staging.  The reference converts and copies every entry of the batch dict with a
blocking ``.float().cuda()`` from pageable memory (mono/apis/trainer.py:19-29) -- ~120 MB per step at
B=12 192x640, serialised with the compute stream.  ``DevicePrefetcher`` wraps any loader of batch dicts:
the next batch is copied from pinned memory on a side HIP stream while the current step runs, and is
handed over already on the device (float32; uint8 frames of the 'uint8' wire format stay bytes and are expanded by
``mono.datasets.device_expand`` in batch_processor), so ``change_input_variable`` finds nothing left to copy."""
import torch

from .raw_wire import HOST_KEYS, keeps_dtype


class DevicePrefetcher:
    def __init__(self, loader, device=None):
        self.loader = loader
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.stream = torch.cuda.Stream(device=self.device)
        self.sampler = getattr(loader, "sampler", None)

    def __len__(self):
        return len(self.loader)

    def _stage(self, batch):
        out = {}
        with torch.cuda.stream(self.stream):
            for k, v in batch.items():
                if isinstance(v, torch.Tensor) and k in HOST_KEYS:
                    out[k] = v                  # read by the host in the device-side expansion (raw_wire.py)
                elif isinstance(v, torch.Tensor):
                    if not v.is_pinned():
                        v = v.pin_memory()
                    v = v.to(self.device, non_blocking=True)
                    # the byte wire formats stay bytes ("raw_meta" int32, the 'resident' wire's offsets int64) until the device-side
                    # expansion (device_expand.py)
                    out[k] = v if keeps_dtype(k) else v.float()
                else:
                    out[k] = v
        return out

    def __iter__(self):
        it = iter(self.loader)
        try:
            nxt = self._stage(next(it))
        except StopIteration:
            return
        while nxt is not None:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
            cur = nxt
            for v in cur.values():
                if isinstance(v, torch.Tensor) and v.is_cuda:
                    v.record_stream(torch.cuda.current_stream(self.device))
            try:
                nxt = self._stage(next(it))
            except StopIteration:
                nxt = None
            yield cur
