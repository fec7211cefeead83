"""Bit-packed instance masks: 1 bit per pixel instead of the reference's float32 (`include/yolact_hip.h`, "bit-packed instance masks").

Layout: `bits` int64 `[n, H, Wq]`, `Wq = ceil(W / 64)`, contiguous.  Bit `k` (LSB = 0) of word `j` of row `y` of mask `i` is pixel
`(y, 64 * j + k)`; bits at `x >= W` are zero.  100 masks at 480 x 640 are 3.84 MB instead of 122.88 MB.  `pack_reference` /
`unpack_reference` below state that layout in numpy (host only; what the tests compare the kernels with).

`after_nms(..., packed=True)` produces a `PackedMasks` directly (`ym_after_nms_batch_packed`: the dense tensor never exists), and
`mask_iou`, `prep_metrics`, `rle_encode`, `MakeJson.add_mask`, `draw_img`, `draw_batch` and `cutout_mattes` accept one wherever
they accept the dense tensor, with bit-identical results.  The words live on the device; there is no CPU path.
"""
import ctypes

import numpy as np
import torch

from .. import hip


def pack_reference(masks):
    """numpy: masks `[..., H, W]` of any dtype (nonzero = foreground) -> int64 words `[..., H, ceil(W / 64)]`."""
    m = np.asarray(masks) != 0
    w = m.shape[-1]
    wq = (w + 63) // 64
    padded = np.zeros(m.shape[:-1] + (wq * 64,), dtype=bool)
    padded[..., :w] = m
    by = np.packbits(padded, axis=-1, bitorder='little')                 # byte b of a row = pixels 8b .. 8b+7, LSB first
    return np.ascontiguousarray(by).view('<u8').astype(np.uint64).view(np.int64)


def unpack_reference(bits, width):
    """numpy: int64 words `[..., H, Wq]` -> uint8 `[..., H, width]` in {0, 1}."""
    b = np.ascontiguousarray(np.asarray(bits)).view(np.uint64).astype('<u8')
    by = b.view(np.uint8).reshape(b.shape[:-1] + (b.shape[-1] * 8,))
    return np.unpackbits(by, axis=-1, bitorder='little')[..., :width]


def _need_cuda(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f'yolact_minimal_amd.utils.packed_masks.{what} needs a CUDA (HIP) tensor; there is no CPU path.')


class PackedMasks:
    """Device-resident bit-packed masks.  `bits` is int64 `[n, H, Wq]` (or `[B, max_det, H, Wq]` in the padded batch form, or
    `[H, Wq]` for one mask); indexing works on the leading (detection) axis like on the dense tensor."""

    __slots__ = ('bits', 'height', 'width')

    @classmethod
    def _wrap(cls, bits, height, width):
        """Internal: words this package has just allocated with the right shape (no checks; after_nms is a 20 us call)."""
        self = object.__new__(cls)
        self.bits, self.height, self.width = bits, height, width
        return self

    def __init__(self, bits, height, width):
        _need_cuda(bits, 'PackedMasks')
        wq = (int(width) + 63) // 64
        if bits.dtype != torch.int64 or bits.dim() < 2 or tuple(bits.shape[-2:]) != (int(height), wq):
            raise RuntimeError(f'PackedMasks: int64 [..., {height}, {wq}] words expected for {height} x {width} masks, got {bits.dtype} '
                               f'{tuple(bits.shape)}')
        self.bits, self.height, self.width = bits, int(height), int(width)

    # ---- tensor-like surface -------------------------------------------------------------------------------------------
    @property
    def shape(self):
        return tuple(self.bits.shape[:-2]) + (self.height, self.width)

    @property
    def device(self):
        return self.bits.device

    @property
    def is_cuda(self):
        return True

    @property
    def nbytes(self):
        return self.bits.numel() * 8

    def dim(self):
        return self.bits.dim()

    def __len__(self):
        return self.bits.shape[0]

    def __getitem__(self, idx):
        """An int, slice, index tensor or bool tensor over the detection axis (what `[:n]` and the `visual_thre` filter need)."""
        if isinstance(idx, tuple) or idx is Ellipsis or idx is None:
            raise IndexError('PackedMasks: index the leading (detection) axis only')
        if self.bits.dim() < 3:
            raise IndexError('PackedMasks: a single mask has no detection axis')
        return PackedMasks._wrap(self.bits[idx], self.height, self.width)    # (rows of valid words are valid words)

    def contiguous(self):
        return self if self.bits.is_contiguous() else PackedMasks(self.bits.contiguous(), self.height, self.width)

    def record_stream(self, stream):
        self.bits.record_stream(stream)

    def __repr__(self):
        return f'PackedMasks(shape={self.shape}, device={self.device}, nbytes={self.nbytes})'

    # ---- conversions ---------------------------------------------------------------------------------------------------
    def _count(self):
        n = 1
        for d in self.bits.shape[:-2]:
            n *= d
        return n

    def dense(self, dtype=torch.float32):
        """The reference's tensor on the device: `[..., H, W]`, exactly 0 / 1 (`ym_unpack_masks`)."""
        out = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        n = self._count()
        if n:
            with torch.cuda.device(self.device):
                hip.check(hip.lib().ym_unpack_masks(hip.ptr(self.bits.contiguous(), torch.int64), n, self.height, self.width, hip.ptr(out),
                                                    hip.stream_ptr()), 'ym_unpack_masks')
        return out if dtype == torch.float32 else out.to(dtype)

    def numpy(self):
        """uint8 `[..., H, W]` on the host: the WORDS cross PCIe (1/32 of the dense bytes), numpy unpacks them.  This is the array
        `pycocotools.mask.encode` wants."""
        return unpack_reference(self.bits.cpu().numpy(), self.width)

    @staticmethod
    def pack(masks):
        """Dense `[..., H, W]` float32 / uint8 / bool device tensor (nonzero = foreground) -> PackedMasks (`ym_pack_masks`)."""
        _need_cuda(masks, 'PackedMasks.pack')
        if masks.dim() < 2:
            raise RuntimeError(f'PackedMasks.pack: [..., H, W] masks expected, got {tuple(masks.shape)}')
        if masks.dtype == torch.bool:
            masks = masks.contiguous().view(torch.uint8)
        elif masks.dtype not in (torch.float32, torch.uint8):
            masks = masks.to(torch.float32)
        m = masks.contiguous()
        h, w = m.shape[-2:]
        bits = torch.empty(tuple(m.shape[:-1]) + ((w + 63) // 64,), dtype=torch.int64, device=m.device)
        n = m.numel() // (h * w) if h * w else 0
        if n:
            with torch.cuda.device(m.device):
                hip.check(hip.lib().ym_pack_masks(hip.ptr(m, m.dtype), int(m.dtype == torch.uint8), n, h, w, hip.ptr(bits, torch.int64),
                                                  hip.stream_ptr()), 'ym_pack_masks')
        return PackedMasks(bits, h, w)


def as_packed(masks, height, width):
    """`masks` as `PackedMasks` of `height` x `width`: itself, or a dense tensor (`[n, H, W]` or flattened `[n, H*W]`) packed."""
    if isinstance(masks, PackedMasks):
        if (masks.height, masks.width) != (height, width):
            raise RuntimeError(f'packed masks of {masks.height} x {masks.width} where {height} x {width} is expected')
        return masks
    _need_cuda(masks, 'as_packed')
    return PackedMasks.pack(masks.reshape(-1, height, width))


def mask_iou_packed(mask1, mask2, to_cpu=True):
    """`box_utils.mask_iou` with a `PackedMasks` on either side (a dense other side, [g, H, W] or [g, H*W], is packed first):
    `ym_mask_iou_packed`, the same exact integer counts as the dense call, so the same floats (0/0 -> NaN)."""
    ref = mask1 if isinstance(mask1, PackedMasks) else mask2
    h, w = ref.height, ref.width
    a = mask1 if mask1 is ref else as_packed(mask1, h, w)
    b = mask2 if isinstance(mask2, PackedMasks) else as_packed(mask2, h, w)
    if (b.height, b.width) != (h, w) or a.bits.dim() != 3 or b.bits.dim() != 3 or a.bits.device != b.bits.device:
        raise RuntimeError(f'mask_iou: [n, H, W] x [g, H, W] masks of one size on one device expected, got {a.shape} on {a.device} x '
                           f'{b.shape} on {b.device}')
    abits = a.bits if a.bits.is_contiguous() else a.bits.contiguous()
    bbits = b.bits if b.bits.is_contiguous() else b.bits.contiguous()
    n, g, words = abits.shape[0], bbits.shape[0], h * abits.shape[2]
    out = torch.empty(n, g, device=abits.device, dtype=torch.float32)
    if n and g:
        L = hip.lib()
        nb = L.ym_mask_iou_packed_workspace_bytes(n, g, words)
        ws = torch.empty(nb, device=abits.device, dtype=torch.uint8)
        hip.check(L.ym_mask_iou_packed(hip.ptr(abits, torch.int64), n, hip.ptr(bbits, torch.int64), g, words, hip.ptr(out),
                                       ctypes.c_void_p(ws.data_ptr()), nb, hip.stream_ptr()), 'ym_mask_iou_packed')
    return out.cpu() if to_cpu else out
