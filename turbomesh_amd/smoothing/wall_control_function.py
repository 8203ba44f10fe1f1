"""Mirror of reference src/core/smoothing/wall_control_function.zig: Algorithm = laplace | white -- and the two kinds the
library adds for any topology: thomas_middlecoff (block-local field from the block's own edges, evaluated on the device and
frozen) and prescribed (the caller's per-node field)."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .. import _capi


@dataclass
class White:
    """wall_control_function.zig:56-68"""

    ds_target: float
    theta_target: float = 0.5 * math.pi


@dataclass
class Algorithm:
    """wall_control_function.zig:16-20: union(enum){laplace: void, white: White} + thomas_middlecoff: void, prescribed: fields"""

    white: "White | None" = None
    kind: "int | None" = None        # None: laplace or white, by `white`
    fields: "list | None" = None     # prescribed: one (ni, nj, 2) array per block, P then Q; Smoother sets them after create

    @classmethod
    def laplace(cls):
        return cls(None)

    @classmethod
    def thomas_middlecoff(cls):
        return cls(None, _capi.TM_CF_THOMAS_MIDDLECOFF)

    @classmethod
    def prescribed(cls, fields):
        fields = [np.ascontiguousarray(f, dtype=np.float64) for f in fields]
        for f in fields:
            if f.ndim != 3 or f.shape[2] != 2:
                raise ValueError(f"a prescribed control function is one (ni, nj, 2) array per block, got {f.shape}")
        return cls(None, _capi.TM_CF_PRESCRIBED, fields)

    def c_struct(self):
        if self.kind is not None:
            return _capi.tm_control_fn(self.kind, 0, 0.0, 0.0)
        if self.white is None:
            return _capi.tm_control_fn(_capi.TM_CF_LAPLACE, 0, 0.0, 0.0)
        return _capi.tm_control_fn(_capi.TM_CF_WHITE, 0, self.white.ds_target, self.white.theta_target)
