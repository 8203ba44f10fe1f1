"""Spanwise stacking: K smoothed 2-D cuts -> the blocks of a 3-D mesh (include/tm_hip.h, "3-D from 2-D cuts"; the reference's roadmap
items "extension to 3D based on meshed 2d cuts" and "rotational configurations").

A layer k of a 3-D block is a fixed linear combination of the same node in the K cuts, v[k] = sum_c A[k][c] v_c: linear or
natural-cubic-spline weights from the span positions alone, planar (x, y, s) or cylindrical (x, r sin(theta), r cos(theta)) output.

    st = Stack(span=[0.0, 0.5, 1.0], layers=layers_from([0.0, 0.5, 1.0], 33))
    X, Y, Z = st.block(cuts, b)            # cuts: a list of Mesh (uploaded per call) or of Smoother (resident coordinates)
    st.mesh3d(cuts).write("blade.xyz")     # multi-block 3-D PLOT3D

Evaluated on the MI355X (kernel K11); `host=True` evaluates the same definition on the CPU (lists of Mesh only)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

from . import _capi
from . import clustering as cluster

INTERPOLATION = {"linear": _capi.TM_STACK_LINEAR, "cubic": _capi.TM_STACK_CUBIC}
MAPPING = {"planar": _capi.TM_STACK_PLANAR, "cylindrical": _capi.TM_STACK_CYLINDRICAL}


def layers_from(span, nk, clustering=None):
    """nk layer coordinates over the span of the cuts: s_k = z0 + u_k (z_{K-1} - z0), u = clustering.create(clustering, nk) (uniform by
    default); the end layers are z0 and z_{K-1} exactly, so they reproduce the end cuts.  nk = 1 gives the single layer z0."""
    z = np.asarray(span, dtype=np.float64)
    if z.ndim != 1 or z.size < 2:
        raise ValueError("span: at least two cut positions")
    if nk < 1:
        raise ValueError("at least one layer")
    if nk == 1:
        return np.array([z[0]])
    u = np.asarray(cluster.create(clustering if clustering is not None else cluster.Uniform(), nk), dtype=np.float64)
    s = np.clip(z[0] + u * (z[-1] - z[0]), z[0], z[-1])
    s[0], s[-1] = z[0], z[-1]
    return s


def quality_of_planes(X, Y, Z, block=0, field=False):
    """quality.Quality3d of any 3-D block given as (nk, nj, ni) arrays (PLOT3D order: what Stack.block returned, or a file read with
    output.read_plot3d_3d), evaluated on the CPU (tm_quality3d_planes_host: no GPU needed).  field=True: (record, per-cell min of the
    oriented scaled Jacobian as a (nk-1, nj-1, ni-1) array)."""
    from . import quality as _quality

    X, Y, Z = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, Y, Z))
    if X.ndim != 3 or Y.shape != X.shape or Z.shape != X.shape:
        raise ValueError("X, Y, Z: three (nk, nj, ni) arrays of one shape")
    nk, nj, ni = X.shape
    q = _capi.tm_quality3d()
    f = np.empty((max(0, nk - 1), max(0, nj - 1), max(0, ni - 1)), dtype=np.float64) if field else None
    _capi.check(_capi.lib().tm_quality3d_planes_host(_capi.f64ptr(X), _capi.f64ptr(Y), _capi.f64ptr(Z), ni, nj, nk, block, C.byref(q),
                                                     _capi.f64ptr(f) if field else None))
    rec = _quality.Quality3d.from_struct(q)
    return (rec, f) if field else rec


@dataclass
class Mesh3d:
    """Blocks of a stacked mesh: per block the X, Y, Z coordinates as (nk, nj, ni) arrays (PLOT3D order, i fastest)."""

    names: List[str] = field(default_factory=list)
    blocks: List[Tuple[np.ndarray, np.ndarray, np.ndarray]] = field(default_factory=list)

    def sizes(self):
        return [(x.shape[2], x.shape[1], x.shape[0]) for x, _, _ in self.blocks]

    def write(self, filename):
        """Multi-block 3-D PLOT3D (output.write_plot3d_3d)."""
        from . import output

        output._format_of(filename)
        output.write_plot3d_3d(filename, self.sizes(), self.blocks)


class Stack:
    """tm_stack_opt + the calls that take it."""

    def __init__(self, span, layers, interpolation="cubic", mapping="planar"):
        if interpolation not in INTERPOLATION:
            raise ValueError(f"interpolation {interpolation!r}: one of {sorted(INTERPOLATION)}")
        if mapping not in MAPPING:
            raise ValueError(f"mapping {mapping!r}: one of {sorted(MAPPING)}")
        self.span = np.ascontiguousarray(span, dtype=np.float64).reshape(-1)
        self.layers = np.ascontiguousarray(layers, dtype=np.float64).reshape(-1)
        self.interpolation, self.mapping = interpolation, mapping
        self._opt = _capi.tm_stack_opt(self.span.size, _capi.f64ptr(self.span), self.layers.size, _capi.f64ptr(self.layers),
                                       INTERPOLATION[interpolation], MAPPING[mapping])

    @property
    def ncuts(self):
        return int(self.span.size)

    @property
    def nlayers(self):
        return int(self.layers.size)

    def weights(self):
        """The (nlayers, ncuts) weight matrix (tm_stack_weights: host only)."""
        w = np.empty((max(1, self.nlayers), max(1, self.ncuts)), dtype=np.float64)
        _capi.check(_capi.lib().tm_stack_weights(C.byref(self._opt), _capi.f64ptr(w)))
        return w[:self.nlayers, :self.ncuts]

    def _check_count(self, cuts):
        if len(cuts) != self.ncuts:
            raise ValueError(f"{len(cuts)} cuts for {self.ncuts} span positions")

    def block(self, cuts, b, k_begin=0, k_count=None, host=False):
        """Layers [k_begin, k_begin + k_count) of block b as three (k_count, nj, ni) arrays.  cuts: one discrete.Mesh per cut (host
        coordinates, uploaded per call: tm_stack_block; host=True: tm_stack_block_host, no GPU) or one smooth.Smoother per cut (the
        coordinates resident in the handles: tm_stack_smoothers)."""
        self._check_count(cuts)
        if k_count is None:
            k_count = self.nlayers - k_begin
        resident = all(hasattr(c, "_h") for c in cuts)
        meshes = [c._mesh for c in cuts] if resident else cuts
        ni, nj = meshes[0].blocks[b].points.size
        out = [np.empty((max(0, k_count), nj, ni), dtype=np.float64) for _ in range(3)]
        ptrs = [_capi.f64ptr(o) for o in out]
        L = _capi.lib()
        if resident:
            if host:
                raise ValueError("host=True evaluates host coordinates: pass the meshes, not the handles")
            handles = (C.c_void_p * len(cuts))(*[c._h for c in cuts])
            _capi.check(L.tm_stack_smoothers(handles, C.byref(self._opt), b, k_begin, k_count, *ptrs))
        else:
            descs = [_capi.MeshDesc(m) for m in meshes]
            arr = (C.POINTER(_capi.tm_mesh_desc) * len(descs))(*[C.pointer(d.desc) for d in descs])
            fn = L.tm_stack_block_host if host else L.tm_stack_block
            _capi.check(fn(arr, C.byref(self._opt), b, k_begin, k_count, *ptrs))
        return tuple(out)

    def quality(self, cuts, host=False):
        """(per_block, total): the 3-D quality report of every stacked block (quality.Quality3d) and their total -- negative and degenerate
        hexahedra ACROSS layers, which the 2-D report of the cuts cannot see.  Evaluated on the device straight from the cuts (kernel K12:
        the 3-D block is never stored); cuts as in block(): Mesh (tm_stack_quality; host=True: tm_stack_quality_host, no GPU) or Smoother
        (tm_stack_smoothers_quality, the resident coordinates)."""
        from . import quality as _quality

        self._check_count(cuts)
        resident = all(hasattr(c, "_h") for c in cuts)
        meshes = [c._mesh for c in cuts] if resident else cuts
        L = _capi.lib()
        per_block = []
        if resident:
            if host:
                raise ValueError("host=True evaluates host coordinates: pass the meshes, not the handles")
            handles = (C.c_void_p * len(cuts))(*[c._h for c in cuts])
        else:
            descs = [_capi.MeshDesc(m) for m in meshes]
            arr = (C.POINTER(_capi.tm_mesh_desc) * len(descs))(*[C.pointer(d.desc) for d in descs])
        for b in range(len(meshes[0].blocks)):
            q = _capi.tm_quality3d()
            if resident:
                _capi.check(L.tm_stack_smoothers_quality(handles, C.byref(self._opt), b, C.byref(q)))
            else:
                _capi.check((L.tm_stack_quality_host if host else L.tm_stack_quality)(arr, C.byref(self._opt), b, C.byref(q)))
            per_block.append(_quality.Quality3d.from_struct(q))
        return per_block, _quality.total_3d(per_block)

    def quality_field(self, cuts, b, k_begin=0, k_count=None):
        """Per-cell minimum of the oriented scaled Jacobian of block b, cell layers [k_begin, k_begin + k_count), as a (k_count, nj-1, ni-1)
        array (NaN for degenerate cells).  cuts: one smooth.Smoother per cut (tm_stack_smoothers_quality_field)."""
        self._check_count(cuts)
        if not all(hasattr(c, "_h") for c in cuts):
            raise ValueError("quality_field reads the coordinates resident in handles: pass one Smoother per cut")
        if k_count is None:
            k_count = self.nlayers - 1 - k_begin
        ni, nj = cuts[0]._mesh.blocks[b].points.size
        out = np.empty((max(0, k_count), max(0, nj - 1), max(0, ni - 1)), dtype=np.float64)
        handles = (C.c_void_p * len(cuts))(*[c._h for c in cuts])
        _capi.check(_capi.lib().tm_stack_smoothers_quality_field(handles, C.byref(self._opt), b, k_begin, k_count, _capi.f64ptr(out)))
        return out

    def mesh3d(self, cuts, host=False) -> Mesh3d:
        """Every block of the cuts, all layers."""
        self._check_count(cuts)
        first = cuts[0]._mesh if hasattr(cuts[0], "_h") else cuts[0]
        m = Mesh3d()
        for b, name in enumerate(first.names):
            m.names.append(name)
            m.blocks.append(self.block(cuts, b, host=host))
        return m
