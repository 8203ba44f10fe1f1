"""Mesh quality report: folded / degenerate cells, scaled Jacobian (worst cell, histogram), corner angles, aspect ratio, edge
growth and areas, per block and for the whole mesh (include/tm_hip.h, "mesh quality"; the reference has no such report).

`mesh(m)` evaluates on the MI355X (tm_mesh_quality), `mesh(m, host=True)` the same definitions on the CPU
(tm_mesh_quality_host: no GPU needed, every field but the summed total_area equal bit for bit).  A `Smoother` reports on the
coordinates resident in its handle (`Smoother.quality()`, `Smoother.quality_field(block)`)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Tuple

from . import _capi


@dataclass
class Quality:
    """tm_quality as a record."""

    cells: int
    inverted: int
    degenerate: int
    orientation: int           # +1 / -1: handedness of the block (sign of the summed cell areas); 0: none, or blocks differ (total)
    min_scaled_jacobian: float
    worst_block: int
    worst_i: int
    worst_j: int
    min_angle_deg: float
    max_angle_deg: float
    max_aspect: float
    max_growth_i: float
    max_growth_j: float
    min_area: float
    max_area: float
    total_area: float
    hist: Tuple[int, ...]      # valid cells by min scaled Jacobian, bins [k/10, (k+1)/10)

    @classmethod
    def from_struct(cls, q: "_capi.tm_quality") -> "Quality":
        return cls(int(q.cells), int(q.inverted), int(q.degenerate), int(q.orientation), float(q.min_scaled_jacobian), int(q.worst_block),
                   int(q.worst_i), int(q.worst_j), float(q.min_angle_deg), float(q.max_angle_deg), float(q.max_aspect), float(q.max_growth_i),
                   float(q.max_growth_j), float(q.min_area), float(q.max_area), float(q.total_area), tuple(int(h) for h in q.hist))

    @property
    def ok(self) -> bool:
        return self.inverted == 0 and self.degenerate == 0

    def line(self, name: str) -> str:
        """One log line: name, cells, inverted, degenerate, min scaled Jacobian with its cell, angle range, max aspect, growth."""
        return (f"{name}: cells {self.cells} inverted {self.inverted} degenerate {self.degenerate} "
                f"min scaled jacobian {self.min_scaled_jacobian:.4f} at (block {self.worst_block}, i {self.worst_i}, j {self.worst_j}) "
                f"angles {self.min_angle_deg:.2f}..{self.max_angle_deg:.2f} deg max aspect {self.max_aspect:.1f} "
                f"max growth i {self.max_growth_i:.3f} j {self.max_growth_j:.3f}")


@dataclass
class Quality3d:
    """tm_quality3d as a record: the hexahedra of a stacked block (include/tm_hip.h, "3-D quality of stacked blocks")."""

    cells: int
    inverted: int
    degenerate: int
    orientation: int           # +1 / -1: handedness of the block (sign of the summed cell volumes); 0: none, or blocks differ (total)
    min_scaled_jacobian: float
    worst_block: int
    worst_i: int
    worst_j: int
    worst_k: int
    max_aspect: float
    max_growth_k: float
    min_volume: float
    max_volume: float
    total_volume: float
    hist: Tuple[int, ...]      # valid cells by min scaled Jacobian, bins [k/10, (k+1)/10)

    @classmethod
    def from_struct(cls, q: "_capi.tm_quality3d") -> "Quality3d":
        return cls(int(q.cells), int(q.inverted), int(q.degenerate), int(q.orientation), float(q.min_scaled_jacobian), int(q.worst_block),
                   int(q.worst_i), int(q.worst_j), int(q.worst_k), float(q.max_aspect), float(q.max_growth_k), float(q.min_volume),
                   float(q.max_volume), float(q.total_volume), tuple(int(h) for h in q.hist))

    @property
    def ok(self) -> bool:
        return self.inverted == 0 and self.degenerate == 0

    def line(self, name: str) -> str:
        """One log line: name, cells, inverted, degenerate, min scaled Jacobian with its cell, max aspect, spanwise growth, volumes."""
        return (f"{name}: hexahedra {self.cells} inverted {self.inverted} degenerate {self.degenerate} "
                f"min scaled jacobian {self.min_scaled_jacobian:.4f} at (block {self.worst_block}, i {self.worst_i}, j {self.worst_j}, k {self.worst_k}) "
                f"max aspect {self.max_aspect:.1f} max growth k {self.max_growth_k:.3f} "
                f"volume {self.min_volume:.3e}..{self.max_volume:.3e} total {self.total_volume:.6e}")


def total_3d(per_block: List[Quality3d]) -> Quality3d:
    """tm_quality3d_total of the blocks' records (host only)."""
    arr = (_capi.tm_quality3d * max(1, len(per_block)))()
    for k, q in enumerate(per_block):
        arr[k] = _capi.tm_quality3d(q.cells, q.inverted, q.degenerate, q.orientation, 0, q.min_scaled_jacobian, q.worst_block, q.worst_i, q.worst_j,
                                    q.worst_k, q.max_aspect, q.max_growth_k, q.min_volume, q.max_volume, q.total_volume, (C.c_uint64 * 10)(*q.hist))
    total = _capi.tm_quality3d()
    _capi.check(_capi.lib().tm_quality3d_total(arr, len(per_block), C.byref(total)))
    return Quality3d.from_struct(total)


def log_report_3d(logger, names, per_block, total, stage="stack"):
    """One line per block and a total, on `logger` at INFO; every line starts with `stage`."""
    for name, q in zip(names, per_block):
        logger.info("%s", q.line(f"{stage} {name}"))
    logger.info("%s", total.line(f"{stage} total"))


@dataclass
class HoQuality:
    """tm_ho_quality as a record: the curved elements of an elevated block (include/tm_hip.h, "high-order elements").  The scaled
    Jacobian is sampled at the element's nodes: necessary for validity, not sufficient -- HoCertificate is the sufficient test."""

    elements: int
    invalid: int
    orientation: int           # +1 / -1: handedness of the block (sign of the summed corner-cell areas); 0: none, or blocks differ (total)
    order: int
    min_scaled_jacobian: float
    worst_block: int
    worst_e: int
    worst_f: int
    min_jacobian: float
    max_jacobian: float
    hist: Tuple[int, ...]      # valid elements by scaled Jacobian, bins [k/10, (k+1)/10)

    @classmethod
    def from_struct(cls, q: "_capi.tm_ho_quality") -> "HoQuality":
        return cls(int(q.elements), int(q.invalid), int(q.orientation), int(q.order), float(q.min_scaled_jacobian), int(q.worst_block),
                   int(q.worst_e), int(q.worst_f), float(q.min_jacobian), float(q.max_jacobian), tuple(int(h) for h in q.hist))

    def to_struct(self) -> "_capi.tm_ho_quality":
        return _capi.tm_ho_quality(self.elements, self.invalid, self.orientation, self.order, self.min_scaled_jacobian, self.worst_block,
                                   self.worst_e, self.worst_f, self.min_jacobian, self.max_jacobian, (C.c_uint64 * 10)(*self.hist))

    @property
    def ok(self) -> bool:
        return self.invalid == 0

    def line(self, name: str) -> str:
        """One log line: name, order, elements, invalid, min scaled Jacobian with its element, Jacobian range."""
        return (f"{name}: order {self.order} elements {self.elements} invalid {self.invalid} "
                f"min scaled jacobian {self.min_scaled_jacobian:.4f} at (block {self.worst_block}, e {self.worst_e}, f {self.worst_f}) "
                f"jacobian {self.min_jacobian:.3e}..{self.max_jacobian:.3e}")


def total_ho(per_block: List[HoQuality]) -> HoQuality:
    """tm_ho_quality_total of the blocks' records (host only)."""
    arr = (_capi.tm_ho_quality * max(1, len(per_block)))()
    for k, q in enumerate(per_block):
        arr[k] = q.to_struct()
    total = _capi.tm_ho_quality()
    _capi.check(_capi.lib().tm_ho_quality_total(arr, len(per_block), C.byref(total)))
    return HoQuality.from_struct(total)


def log_report_ho(logger, names, per_block, total, stage="elevate"):
    """One line per block and a total, on `logger` at INFO; every line starts with `stage`."""
    for name, q in zip(names, per_block):
        logger.info("%s", q.line(f"{stage} {name}"))
    logger.info("%s", total.line(f"{stage} total"))


@dataclass
class HoQuality3d:
    """tm_ho3_quality as a record: the curved hexahedra of a stacked block judged at their nodes (include/tm_hip.h, "high-order hexahedra
    of stacked blocks").  Sampled at the nodes: necessary for valid elements, not sufficient."""

    elements: int
    invalid: int
    orientation: int
    order: int
    min_scaled_jacobian: float
    worst_block: int
    worst_e: int
    worst_f: int
    worst_g: int
    min_jacobian: float
    max_jacobian: float
    hist: Tuple[int, ...]      # valid elements by scaled Jacobian, bins [k/10, (k+1)/10)

    @classmethod
    def from_struct(cls, q: "_capi.tm_ho3_quality") -> "HoQuality3d":
        return cls(int(q.elements), int(q.invalid), int(q.orientation), int(q.order), float(q.min_scaled_jacobian), int(q.worst_block),
                   int(q.worst_e), int(q.worst_f), int(q.worst_g), float(q.min_jacobian), float(q.max_jacobian), tuple(int(h) for h in q.hist))

    def to_struct(self) -> "_capi.tm_ho3_quality":
        return _capi.tm_ho3_quality(self.elements, self.invalid, self.orientation, self.order, self.min_scaled_jacobian, self.worst_block,
                                    self.worst_e, self.worst_f, self.worst_g, self.min_jacobian, self.max_jacobian, (C.c_uint64 * 10)(*self.hist))

    @property
    def ok(self) -> bool:
        return self.invalid == 0

    def line(self, name: str) -> str:
        """One log line: name, order, elements, invalid, min scaled Jacobian with its element, Jacobian range."""
        return (f"{name}: order {self.order} elements {self.elements} invalid {self.invalid} "
                f"min scaled jacobian {self.min_scaled_jacobian:.4f} at (block {self.worst_block}, e {self.worst_e}, f {self.worst_f}, g {self.worst_g}) "
                f"jacobian {self.min_jacobian:.3e}..{self.max_jacobian:.3e}")


def total_ho3(per_block: List[HoQuality3d]) -> HoQuality3d:
    """tm_ho3_quality_total of the blocks' records (host only)."""
    arr = (_capi.tm_ho3_quality * max(1, len(per_block)))()
    for k, q in enumerate(per_block):
        arr[k] = q.to_struct()
    total = _capi.tm_ho3_quality()
    _capi.check(_capi.lib().tm_ho3_quality_total(arr, len(per_block), C.byref(total)))
    return HoQuality3d.from_struct(total)


def log_report_ho3(logger, names, per_block, total, stage="elevate3d"):
    """One line per block and a total, on `logger` at INFO; every line starts with `stage`."""
    for name, q in zip(names, per_block):
        logger.info("%s", q.line(f"{stage} {name}"))
    logger.info("%s", total.line(f"{stage} total"))


@dataclass
class HoCertificate:
    """tm_ho_certificate as a record: the elements of a block judged by the Bernstein coefficients of their Jacobian (include/tm_hip.h,
    "high-order elements: certificate").  proven: o*J > 0 on the whole element; invalid: o*J <= 0 at a point; undecided: neither shown
    within max_depth subdivisions.  hidden_invalid counts the invalid elements that the nodal record (HoQuality) calls valid."""

    elements: int
    proven: int
    invalid: int
    undecided: int
    hidden_invalid: int
    orientation: int
    order: int
    max_depth: int             # -1: blocks differ (total)
    has_unproven: bool
    decided_at: Tuple[int, ...]   # proven and invalid elements by the subdivision level that decided them
    min_scaled_bound: float    # min over proven elements of the certified lower bound of min J / max J
    worst_block: int
    worst_e: int
    worst_f: int
    first_unproven_block: int
    first_unproven_e: int
    first_unproven_f: int

    @classmethod
    def from_struct(cls, c: "_capi.tm_ho_certificate") -> "HoCertificate":
        return cls(int(c.elements), int(c.proven), int(c.invalid), int(c.undecided), int(c.hidden_invalid), int(c.orientation), int(c.order),
                   int(c.max_depth), bool(c.has_unproven), tuple(int(d) for d in c.decided_at), float(c.min_scaled_bound), int(c.worst_block),
                   int(c.worst_e), int(c.worst_f), int(c.first_unproven_block), int(c.first_unproven_e), int(c.first_unproven_f))

    def to_struct(self) -> "_capi.tm_ho_certificate":
        return _capi.tm_ho_certificate(self.elements, self.proven, self.invalid, self.undecided, self.hidden_invalid, self.orientation, self.order,
                                       self.max_depth, int(self.has_unproven), (C.c_uint64 * 5)(*self.decided_at), self.min_scaled_bound,
                                       self.worst_block, self.worst_e, self.worst_f, self.first_unproven_block, self.first_unproven_e,
                                       self.first_unproven_f)

    @property
    def ok(self) -> bool:
        return self.proven == self.elements

    def line(self, name: str) -> str:
        """One log line: name, order, depth, the three counts, the hidden folds, the levels and the certified bound."""
        s = (f"{name}: order {self.order} depth {self.max_depth} elements {self.elements} proven {self.proven} invalid {self.invalid} "
             f"undecided {self.undecided} hidden invalid {self.hidden_invalid} decided at {'/'.join(str(d) for d in self.decided_at)} "
             f"min scaled bound {self.min_scaled_bound:.4f} at (block {self.worst_block}, e {self.worst_e}, f {self.worst_f})")
        if self.has_unproven:
            s += f" first unproven (block {self.first_unproven_block}, e {self.first_unproven_e}, f {self.first_unproven_f})"
        return s


def total_ho_certificate(per_block: List[HoCertificate]) -> HoCertificate:
    """tm_ho_certificate_total of the blocks' records (host only)."""
    arr = (_capi.tm_ho_certificate * max(1, len(per_block)))()
    for k, c in enumerate(per_block):
        arr[k] = c.to_struct()
    total = _capi.tm_ho_certificate()
    _capi.check(_capi.lib().tm_ho_certificate_total(arr, len(per_block), C.byref(total)))
    return HoCertificate.from_struct(total)


def log_report_ho_certificate(logger, names, per_block, total, stage="certify"):
    """One line per block and a total, on `logger` at INFO; every line starts with `stage`."""
    for name, c in zip(names, per_block):
        logger.info("%s", c.line(f"{stage} {name}"))
    logger.info("%s", total.line(f"{stage} total"))


@dataclass
class HoCertificate3d:
    """tm_ho3_certificate as a record: the curved hexahedra of a stacked block judged by the Bernstein coefficients of their Jacobian
    (include/tm_hip.h, "high-order hexahedra: certificate").  proven: o*J > 0 on the whole element; invalid: o*J <= 0 at a point;
    undecided: neither shown within max_depth subdivisions.  hidden_invalid counts the invalid elements that the nodal record
    (HoQuality3d) calls valid."""

    elements: int
    proven: int
    invalid: int
    undecided: int
    hidden_invalid: int
    orientation: int
    order: int
    max_depth: int             # -1: blocks differ (total)
    has_unproven: bool
    decided_at: Tuple[int, ...]   # proven and invalid elements by the subdivision level that decided them
    min_scaled_bound: float    # min over proven elements of the certified lower bound of min J / max J
    worst_block: int
    worst_e: int
    worst_f: int
    worst_g: int
    first_unproven_block: int
    first_unproven_e: int
    first_unproven_f: int
    first_unproven_g: int

    @classmethod
    def from_struct(cls, c: "_capi.tm_ho3_certificate") -> "HoCertificate3d":
        return cls(int(c.elements), int(c.proven), int(c.invalid), int(c.undecided), int(c.hidden_invalid), int(c.orientation), int(c.order),
                   int(c.max_depth), bool(c.has_unproven), tuple(int(d) for d in c.decided_at), float(c.min_scaled_bound), int(c.worst_block),
                   int(c.worst_e), int(c.worst_f), int(c.worst_g), int(c.first_unproven_block), int(c.first_unproven_e),
                   int(c.first_unproven_f), int(c.first_unproven_g))

    def to_struct(self) -> "_capi.tm_ho3_certificate":
        return _capi.tm_ho3_certificate(self.elements, self.proven, self.invalid, self.undecided, self.hidden_invalid, self.orientation, self.order,
                                        self.max_depth, int(self.has_unproven), (C.c_uint64 * 4)(*self.decided_at), self.min_scaled_bound,
                                        self.worst_block, self.worst_e, self.worst_f, self.worst_g, self.first_unproven_block,
                                        self.first_unproven_e, self.first_unproven_f, self.first_unproven_g)

    @property
    def ok(self) -> bool:
        return self.proven == self.elements

    def line(self, name: str) -> str:
        """One log line: name, order, depth, the three counts, the hidden folds, the levels and the certified bound."""
        s = (f"{name}: order {self.order} depth {self.max_depth} elements {self.elements} proven {self.proven} invalid {self.invalid} "
             f"undecided {self.undecided} hidden invalid {self.hidden_invalid} decided at {'/'.join(str(d) for d in self.decided_at)} "
             f"min scaled bound {self.min_scaled_bound:.4f} at (block {self.worst_block}, e {self.worst_e}, f {self.worst_f}, g {self.worst_g})")
        if self.has_unproven:
            s += (f" first unproven (block {self.first_unproven_block}, e {self.first_unproven_e}, f {self.first_unproven_f}, "
                  f"g {self.first_unproven_g})")
        return s


def total_ho3_certificate(per_block: List[HoCertificate3d]) -> HoCertificate3d:
    """tm_ho3_certificate_total of the blocks' records (host only)."""
    arr = (_capi.tm_ho3_certificate * max(1, len(per_block)))()
    for k, c in enumerate(per_block):
        arr[k] = c.to_struct()
    total = _capi.tm_ho3_certificate()
    _capi.check(_capi.lib().tm_ho3_certificate_total(arr, len(per_block), C.byref(total)))
    return HoCertificate3d.from_struct(total)


def log_report_ho3_certificate(logger, names, per_block, total, stage="certify3d"):
    """One line per block and a total, on `logger` at INFO; every line starts with `stage`."""
    for name, c in zip(names, per_block):
        logger.info("%s", c.line(f"{stage} {name}"))
    logger.info("%s", total.line(f"{stage} total"))


def records(per_block, total) -> Tuple[List[Quality], Quality]:
    return [Quality.from_struct(q) for q in per_block], Quality.from_struct(total)


def mesh(mesh_data, host: bool = False) -> Tuple[List[Quality], Quality]:
    """(per_block, total) of a discrete.Mesh; host=True evaluates on the CPU."""
    md = _capi.MeshDesc(mesh_data)
    per_block = (_capi.tm_quality * max(1, len(mesh_data.blocks)))()
    total = _capi.tm_quality()
    fn = _capi.lib().tm_mesh_quality_host if host else _capi.lib().tm_mesh_quality
    _capi.check(fn(md.ref(), per_block, C.byref(total)))
    return records(per_block[:len(mesh_data.blocks)], total)


def log_report(logger, names, per_block, total, stage):
    """One line per block and a total, on `logger` at INFO; every line starts with `stage` ("before" / "after")."""
    for name, q in zip(names, per_block):
        logger.info("%s", q.line(f"{stage} {name}"))
    logger.info("%s", total.line(f"{stage} total"))
