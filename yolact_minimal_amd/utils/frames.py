"""A batch of camera frames / dataset images of DIFFERENT sizes in one device allocation: what `val_aug_batch` reads, what the
ragged `draw_batch` reads and returns, what `RequestPipeline.submit_frames` takes (include/yolact_hip.h, "frames of different sizes").

Layout (`frame_layout`): frame b is HWC BGR `[h_b, w_b, 3]` at element `offsets[b]` of one flat buffer, every frame at a multiple
of 256 bytes, in order, not overlapping: the rules of `ragged_layout`'s mask blocks, so one table type (`hip.RaggedImage`) serves both.
"""
import numpy as np
import torch

from .. import hip


def frame_layout(sizes, itemsize=1):
    """`(offsets, total)` in ELEMENTS (bytes for uint8 frames, `itemsize=4`: floats) of one flat buffer that holds the frames
    `[h_b, w_b, 3]` of `sizes` = [(h, w), ...]: every frame starts at a multiple of 256 bytes, `total` ends the last one.
    Pure Python: no GPU, no library."""
    itemsize = int(itemsize)
    if itemsize < 1 or hip.RAGGED_ALIGN_BYTES % itemsize:
        raise RuntimeError(f'frame_layout: itemsize = {itemsize}')
    return hip.aligned_layout('frame_layout', sizes, itemsize, lambda h, w: h * w * 3)


def _frame_size(t, what, dtypes):
    if t.dtype not in dtypes or t.ndim != 3 or t.shape[2] != 3:
        raise RuntimeError(f'{what}: frames are [H, W, 3] arrays of {" / ".join(str(d) for d in dtypes)}, got {t.dtype} {tuple(t.shape)}')
    return int(t.shape[0]), int(t.shape[1])


class FrameBatch:
    """B frames of their own sizes in ONE flat device allocation `data` (uint8; float32 only through `from_tensors`).  `sizes` =
    [(h, w), ...], `offsets` = where each frame starts in `data` (elements), `frames[b]` = the `[h_b, w_b, 3]` view of frame b.
    `len(batch)` = B."""

    __slots__ = ('data', 'sizes', 'offsets', 'frames', '_table')

    def __init__(self, data, sizes):
        """`data`: a flat buffer that holds `frame_layout(sizes, data.element_size())`.  (The constructor itself takes a host buffer
        too -- it only makes views; every consumer refuses a batch that is not on the device.)"""
        sizes = [(int(h), int(w)) for h, w in sizes]
        if not torch.is_tensor(data) or data.dtype not in (torch.uint8, torch.float32) or data.dim() != 1 or not data.is_contiguous():
            raise RuntimeError('FrameBatch: the buffer is a flat contiguous uint8 (or float32) tensor')
        offsets, total = frame_layout(sizes, data.element_size())
        if data.numel() < total:
            raise RuntimeError(f'FrameBatch: {total} elements needed for {sizes}, the buffer has {data.numel()}')
        if data.data_ptr() % 16:
            raise RuntimeError('FrameBatch: the buffer must be 16-byte aligned')
        self.data, self.sizes, self.offsets = data, sizes, offsets
        self.frames = [data[o:o + h * w * 3].view(h, w, 3) for (h, w), o in zip(sizes, offsets)]
        self._table = None

    # ---- construction --------------------------------------------------------------------------------------------------
    @staticmethod
    def _alloc(sizes, dtype, device):
        _, total = frame_layout(sizes, 1 if dtype == torch.uint8 else 4)
        return FrameBatch(torch.empty(total, dtype=dtype, device=device), sizes)

    @classmethod
    def from_numpy(cls, arrays, device):
        """uint8 HWC numpy frames -> a FrameBatch on `device`: packed into ONE pinned host buffer, ONE host-to-device copy."""
        arrays = _as_list(arrays, 'FrameBatch.from_numpy')
        for a in arrays:
            if not isinstance(a, np.ndarray):
                raise RuntimeError('FrameBatch.from_numpy: a list of numpy uint8 [H, W, 3] arrays expected')
        sizes = [_frame_size(a, 'FrameBatch.from_numpy', (np.dtype(np.uint8),)) for a in arrays]
        offsets, total = frame_layout(sizes)
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('yolact_minimal_amd.utils.frames.FrameBatch lives on the device; there is no CPU path.')
        host = torch.empty(total, dtype=torch.uint8).pin_memory()
        view = host.numpy()
        for a, (h, w), o in zip(arrays, sizes, offsets):
            view[o:o + h * w * 3] = a.reshape(-1)
        return cls(host.to(device, non_blocking=True), sizes)

    @classmethod
    def from_tensors(cls, tensors):
        """Device HWC tensors (all uint8 or all float32, one device) -> a FrameBatch: one allocation, B device copies on the current stream."""
        tensors = _as_list(tensors, 'FrameBatch.from_tensors')
        for t in tensors:
            if not torch.is_tensor(t):
                raise RuntimeError('FrameBatch.from_tensors: a list of device [H, W, 3] tensors expected')
        sizes = [_frame_size(t, 'FrameBatch.from_tensors', (torch.uint8, torch.float32)) for t in tensors]
        if any(t.dtype != tensors[0].dtype for t in tensors):
            raise RuntimeError('FrameBatch.from_tensors: the frames of a batch share one dtype')
        if any(not t.is_cuda or t.device != tensors[0].device for t in tensors):
            raise RuntimeError('yolact_minimal_amd.utils.frames.FrameBatch.from_tensors needs CUDA (HIP) tensors on one device; there is '
                               'no CPU path.')
        self = cls._alloc(sizes, tensors[0].dtype, tensors[0].device)
        for dst, t in zip(self.frames, tensors):
            dst.copy_(t)
        return self

    @classmethod
    def empty_like(cls, other):
        """An uninitialised FrameBatch of `other`'s sizes, dtype and device."""
        if not isinstance(other, FrameBatch):
            raise RuntimeError('FrameBatch.empty_like: a FrameBatch expected')
        return cls._alloc(other.sizes, other.data.dtype, other.data.device)

    # ---- surface -------------------------------------------------------------------------------------------------------
    def __len__(self):
        return len(self.sizes)

    @property
    def device(self):
        return self.data.device

    @property
    def dtype(self):
        return self.data.dtype

    def need_cuda(self, what):
        if not self.data.is_cuda:
            raise RuntimeError(f'yolact_minimal_amd.{what} needs the frames on the device (CUDA / HIP); there is no CPU path.')

    def table(self):
        """The C-ABI table `(hip.RaggedImage * B)` of this batch (built once)."""
        if self._table is None:
            self._table = hip.ragged_table(self.sizes, self.offsets)
        return self._table

    def numpy(self):
        """The frames as a list of host arrays: ONE device-to-host copy of the flat buffer."""
        host = self.data.cpu().numpy()
        return [host[o:o + h * w * 3].reshape(h, w, 3) for (h, w), o in zip(self.sizes, self.offsets)]

    def record_stream(self, stream):
        self.data.record_stream(stream)

    def __repr__(self):
        return f'FrameBatch(sizes={self.sizes}, dtype={self.data.dtype}, device={self.data.device})'


def _as_list(seq, what):
    if isinstance(seq, (np.ndarray, torch.Tensor)) or not hasattr(seq, '__len__'):
        raise RuntimeError(f'{what}: a list of [H, W, 3] frames expected')
    seq = list(seq)
    if not 1 <= len(seq) <= hip.RAGGED_MAX_IMAGES:
        raise RuntimeError(f'{what}: 1 .. {hip.RAGGED_MAX_IMAGES} images per call, got {len(seq)}')
    return seq
