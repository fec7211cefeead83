"""Rows of the tuned table (tuned_gfx950.json): the one module that knows their format.  Host-only.

A forward / data-gradient row is [tile_m, tile_n, ksplit, kwaves, stages, tail_tiles, tail_ksplit(, grid_wgs)], the ym_conv_desc
fields of those names; all zeros = the planner's heuristic.  `stages` also picks the kernel family: 0 / 2 register staging, 3
register ring of 3, 22-24 direct-to-LDS ring of 2-4 (with kwaves > 0: the wave kernel with DMA rings), 33 / 34 DMA ring with
pipelined fragments, 42-48 persistent walker, 52-54 weight-stationary 1x1; the last digit is the ring depth.  `grid_wgs` is the
workgroup count of a persistent row (0 = as many as the CUs hold) and the waves per workgroup of a wave-DMA row.
A weight-gradient row (`W_` keys) is [msplit(, lds_buffers)]."""
from typing import NamedTuple


def _checked(row, n):
    row = list(row)
    if len(row) > n or not all(isinstance(v, int) and not isinstance(v, bool) and v >= 0 for v in row):
        # (old detail rows of InferEngine.autotune carried a timing as their eighth field: it must not land in a c_int32)
        raise ValueError(f'tuned entry {row}: at most {n} non-negative integers')
    return row


class ConvPlan(NamedTuple):
    tile_m: int = 0
    tile_n: int = 0
    ksplit: int = 0
    kwaves: int = 0
    stages: int = 0
    tail_tiles: int = 0
    tail_ksplit: int = 0
    grid_wgs: int = 0

    @classmethod
    def from_row(cls, row):
        """Short rows are padded with zeros; a row no launch can take raises ValueError."""
        p = cls(*_checked(row, 8))
        g = p.grid_wgs
        if p.wave_dma and (g not in (0, 1, 2, 4) or (g and g < p.kwaves) or ((p.tail_tiles or p.tail_ksplit) and g not in (0, 4))):
            # (a grid edited over from a persistent row would be rejected by the launch, or silently lose the tail split)
            raise ValueError(f'tuned entry {list(row)}: field 7 of a wave-DMA row is waves per workgroup (0 / 1 / 2 / 4, >= kwaves; 0 / 4 with a tail)')
        return p

    def to_row(self):
        return list(self) if self.grid_wgs else list(self[:7])

    @classmethod
    def of(cls, desc):
        return cls(*(getattr(desc, f) for f in cls._fields))

    def apply(self, desc):
        for f, v in zip(self._fields, self):
            setattr(desc, f, v)

    wave = property(lambda self: self.kwaves > 0)                                   # the K split runs over the waves of a workgroup
    wave_dma = property(lambda self: self.kwaves > 0 and 22 <= self.stages <= 24)   # ... each with a private DMA ring (conv_wdma_f32)
    persistent = property(lambda self: 42 <= self.stages <= 48)                     # the persistent walker (conv_persist.hip)
    weight_stationary = property(lambda self: 52 <= self.stages <= 54)              # the weight-stationary 1x1 kernel
    ring = property(lambda self: self.stages % 10)                                  # depth of the operand ring

    def with_bn_sums(self):
        """For a launch with fused BatchNorm sums, which the persistent walker does not carry: 42 -> 22, other persistent -> 23."""
        return self._replace(stages=22 if self.stages == 42 else 23, grid_wgs=0) if self.persistent else self


def from_entry(row, cls=ConvPlan):
    """`cls.from_row(row)`, or None for a shape without a row."""
    return None if row is None else cls.from_row(row)


class WgradPlan(NamedTuple):
    msplit: int = 0
    lds_buffers: int = 2

    @classmethod
    def from_row(cls, row):
        return cls(*_checked(row, 2))

    def to_row(self):
        return list(self)

    def apply(self, desc):
        desc.msplit, desc.lds_buffers = self
