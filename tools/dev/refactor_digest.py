"""One line per output of the stages K10 .. K19 and of the entry points that bring their own device memory: the sha256 of what came
back, or the error code and text.  Every reduction of the library is in fixed order and it uses no float atomics, so two builds that
enqueue the same launches print the same lines, byte for byte -- the check behind a change to the host code of those stages
(profiles/report_refactor_digest.txt).  Shapes are those of the GPU tests: handle and host-description entry points, plain and _surf,
the four drivers with a two-stage record combination (K13, K14, K16, K17) on both sides of 256 workgroups.  TM_HIP_LIB selects the
build, as everywhere.

    python tools/dev/refactor_digest.py > digest.txt"""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np

from tests import control_field_reference as cfr
from tests import ho_certify_reference as cr
from tests import stack_reference as sr
from tests import stack_surface_reference as ssr
from tests.meshes import TOPOLOGIES
from turbomesh_amd import _capi, configs, highorder, quality, stack, weld
from turbomesh_amd.discrete import Block2d
from turbomesh_amd.smoothing import smooth, solver

RELAX = solver.Option.hip(inner=solver.Inner.relax)
_ip = C.POINTER(C.c_int32)


def sha(*items):
    h = hashlib.sha256()
    for a in items:
        if a is None:
            h.update(b"none")
        elif isinstance(a, np.ndarray):
            h.update(str(a.shape).encode() + np.ascontiguousarray(a).tobytes())
        elif hasattr(a, "to_struct"):
            h.update(bytes(a.to_struct()))
        elif isinstance(a, C.Structure):
            h.update(bytes(a))
        elif isinstance(a, (list, tuple)):
            h.update(sha(*a).encode())
        else:
            h.update(repr(a).encode())   # dataclasses of numbers: repr is exact for floats
    return h.hexdigest()


def line(label, *items):
    print(label, sha(*items), flush=True)


def error(label, call):
    """code and tm_last_error text of a call that must fail"""
    try:
        call()
    except _capi.TmError as e:
        print(label, "error", e.code, str(e), flush=True)
    except Exception as e:   # refused before the library was asked
        print(label, "python", type(e).__name__, flush=True)
    else:
        print(label, "NO ERROR", flush=True)


def bent_cuts(ni, nj, K):
    return [cfr.single_block_mesh(cfr.bent_clustered(ni, nj, seed=c) + 0.01 * c) for c in range(K)]


def stack_for(K, nk, interpolation, mapping, seed):
    z = sr.spans(K, "uniform" if mapping != "planar" else "nonuniform")
    s = np.sort(sr.layers_with_cuts(z, nk, seed=seed))
    if mapping == "revolution":
        u, x, r, rr = ssr.tables(K, seed=seed)
        return stack.Stack(z, s, interpolation, mapping, surfaces=stack.Surfaces(u, x, r, rr))
    return stack.Stack(z, s, interpolation, mapping)


class Handles:
    """one handle per cut, the coordinates as they were uploaded"""

    def __init__(self, cuts):
        self.cuts = cuts

    def __enter__(self):
        self.sm = [smooth.Smoother(m, RELAX) for m in self.cuts]
        return [s.__enter__() for s in self.sm]

    def __exit__(self, *a):
        for s in self.sm:
            s.__exit__(*a)


def quality_stage():
    for name in ("two_by_two_junction", "channel_periodic_sliding", "strip3_reversed", "plate_le"):
        mesh = TOPOLOGIES[name](None)
        line(f"K10 tm_mesh_quality {name}", *quality.mesh(mesh))
        with smooth.Smoother(mesh, RELAX) as sm:
            sm.iterate(2)
            line(f"K10 tm_smoother_quality {name}", *sm.quality())
            line(f"K10 tm_smoother_quality_field {name}", sm.quality_field(0))
    big = configs.single_block(1025, 1025, perturb=0.25)
    line("K10 tm_mesh_quality perturbed_1025", *quality.mesh(big))
    error("K10 one node row", lambda: quality.mesh(cfr.single_block_mesh(np.zeros((1, 5, 2)))))


def stack_stages():
    for ni, nj, K, nk, interpolation, mapping in ((4, 5, 3, 2, "cubic", "cylindrical"), (33, 34, 2, 5, "linear", "planar"), (67, 130, 16, 33, "cubic", "planar"),
                                                  (40, 37, 8, 7, "cubic", "revolution"), (33, 65, 3, 4, "linear", "revolution")):
        st = stack_for(K, nk, interpolation, mapping, seed=ni + K)
        cuts = bent_cuts(ni, nj, K)
        rev = mapping == "revolution"
        tag = f"{ni}x{nj} K{K} nk{nk} {interpolation} {mapping}"
        line(f"K11 block {tag}", *st.block(cuts, 0, return_outside=rev))
        line(f"K11 block window {tag}", *st.block(cuts, 0, 1, nk - 1, return_outside=rev))
        line(f"K12 quality {tag}", *st.quality(cuts))
        with Handles(cuts) as hs:
            line(f"K11 smoothers {tag}", *st.block(hs, 0, return_outside=rev))
            line(f"K12 smoothers_quality {tag}", *st.quality(hs))
            line(f"K12 smoothers_quality_field {tag}", st.quality_field(hs, 0))
            line(f"K12 smoothers_quality_field window {tag}", st.quality_field(hs, 0, nk - 2, 1))
            error(f"K12 field window past the block {tag}", lambda: st.quality_field(hs, 0, nk - 1, 1))
            error(f"K11 window past the block {tag}", lambda: st.block(hs, 0, nk, 1))
        error(f"K11 host window past the block {tag}", lambda: st.block(cuts, 0, nk, 1))
    # the raw entry points: tables without TM_STACK_REVOLUTION, null options
    st = stack_for(2, 5, "linear", "planar", seed=3)
    rv = stack_for(2, 5, "linear", "revolution", seed=3)
    cuts = bent_cuts(9, 9, 2)
    el = highorder.Elevation(2, "equidistant")
    descs = [_capi.MeshDesc(m) for m in cuts]
    arr = (C.POINTER(_capi.tm_mesh_desc) * 2)(*[C.pointer(d.desc) for d in descs])
    q, c = _capi.tm_ho3_quality(), _capi.tm_ho3_certificate()
    L = _capi.lib()
    error("K16 tables with a planar stack", lambda: _capi.check(L.tm_stack_elevate(arr, C.byref(st._opt), rv.surfaces.ref(), C.byref(el._opt), 0, 0, 0, None, None, None,
                                                                                  C.byref(q), None, None)))
    error("K16 null options", lambda: _capi.check(L.tm_stack_elevate(arr, None, None, C.byref(el._opt), 0, 0, 0, None, None, None, C.byref(q), None, None)))
    error("K17 tables with a planar stack", lambda: _capi.check(L.tm_stack_certify(arr, C.byref(st._opt), rv.surfaces.ref(), C.byref(el._opt), 2, 0, C.byref(c), None, None,
                                                                                  None)))
    error("K17 null options", lambda: _capi.check(L.tm_stack_certify(arr, None, None, C.byref(el._opt), 2, 0, C.byref(c), None, None, None)))
    error("K17 depth", lambda: st.certify(cuts, el, 0, max_depth=99))
    error("K16 order does not divide", lambda: st.elevate(cuts, highorder.Elevation(3, "equidistant"), 0))


def flat_highorder():
    # K13: 16 x 16 = 256 and 17 x 16 = 272 workgroups at p = 1; K14: 519 workgroups on 258 x 259 at p = 1
    for p, ni, nj, dist in ((1, 257, 257, "equidistant"), (1, 273, 257, "gauss_lobatto"), (2, 67, 131, "gauss_lobatto"), (3, 67, 130, "equidistant"),
                            (5, 66, 131, "gauss_lobatto"), (8, 73, 137, "gauss_lobatto"), (4, 5, 5, "gauss_lobatto")):
        mesh = cfr.single_block_mesh(cfr.bent_clustered(ni, nj))
        el = highorder.Elevation(p, dist)
        line(f"K13 tm_ho_elevate p{p} {ni}x{nj} {dist}", *el.block(mesh, 0))
        line(f"K13 tm_ho_elevate report p{p} {ni}x{nj} {dist}", *el.block(mesh, 0, planes=False))
        with smooth.Smoother(mesh, RELAX) as sm:
            line(f"K13 tm_smoother_elevate p{p} {ni}x{nj} {dist}", *el.block(sm, 0))
    for p, ni, nj in ((1, 258, 259), (1, 67, 130), (2, 67, 131), (3, 139, 139), (3, 136, 136), (4, 69, 133), (8, 73, 137), (6, 7, 7)):
        X = cr.dyadic_block(ni, nj, 0.35, seed=1000 * p + ni)   # some elements fail, some subdivide
        mesh = cfr.single_block_mesh(X)
        el = highorder.Elevation(p, "equidistant")
        line(f"K14 tm_ho_certify p{p} {ni}x{nj}", *el.certify(mesh, 0, max_depth=3))
        with smooth.Smoother(mesh, RELAX) as sm:
            line(f"K14 tm_smoother_certify p{p} {ni}x{nj}", *el.certify(sm, 0, max_depth=3))
    error("K13 order does not divide", lambda: highorder.Elevation(3, "equidistant").block(cfr.single_block_mesh(cfr.bent_clustered(9, 9)), 0))


def stacked_highorder():
    # K16 at p = 4 owns 4 x 3 elements per workgroup: 245 x 193 nodes are 16 x 16 = 256 workgroups, 245 x 197 are 16 x 17 = 272.
    # K17 at p = 1 takes 16 elements per workgroup: 33 x 33 x 9 nodes are 512 workgroups, 9 x 9 x 5 are 16.
    for p, ni, nj, K, Eg, interpolation, mapping, dist in ((4, 245, 193, 2, 1, "linear", "planar", "gauss_lobatto"), (4, 245, 197, 2, 1, "linear", "planar", "gauss_lobatto"),
                                                          (4, 245, 197, 3, 1, "cubic", "revolution", "gauss_lobatto"), (2, 17, 29, 3, 2, "cubic", "cylindrical", "equidistant"),
                                                          (3, 31, 16, 8, 3, "cubic", "planar", "gauss_lobatto"), (1, 33, 29, 16, 1, "linear", "revolution", "equidistant")):
        st = stack_for(K, Eg * p + 1, interpolation, mapping, seed=ni + K)
        cuts = bent_cuts(ni, nj, K)
        el = highorder.Elevation(p, dist)
        rev = mapping == "revolution"
        tag = f"p{p} {ni}x{nj} K{K} Eg{Eg} {interpolation} {mapping} {dist}"
        line(f"K16 tm_stack_elevate {tag}", *st.elevate(cuts, el, 0, return_outside=rev))
        line(f"K16 tm_stack_elevate report {tag}", *st.elevate(cuts, el, 0, planes=False))
        line(f"K16 tm_stack_elevate window {tag}", *st.elevate(cuts, el, 0, Eg - 1, 1))
        with Handles(cuts) as hs:
            line(f"K16 tm_stack_smoothers_elevate {tag}", *st.elevate(hs, el, 0, return_outside=rev))
    for p, ni, nj, nk, K, mapping in ((1, 33, 33, 9, 2, "planar"), (1, 33, 33, 9, 3, "revolution"), (1, 9, 9, 5, 2, "cylindrical"), (2, 9, 7, 7, 3, "revolution"),
                                      (3, 7, 10, 4, 2, "planar"), (4, 9, 5, 9, 3, "cylindrical")):
        st = stack_for(K, nk, "cubic" if K == 3 else "linear", mapping, seed=ni + K)
        cuts = bent_cuts(ni, nj, K)
        el = highorder.Elevation(p, "gauss_lobatto")
        tag = f"p{p} {ni}x{nj}x{nk} K{K} {mapping}"
        line(f"K17 tm_stack_certify {tag}", *st.certify(cuts, el, 0, max_depth=2))
        with Handles(cuts) as hs:
            line(f"K17 tm_stack_smoothers_certify {tag}", *st.certify(hs, el, 0, max_depth=2))
    os.environ["TM_HO3_CERT_WINDOW_BYTES"] = str(24 * 33 * 33 * 4)   # three span elements per window
    st = stack_for(2, 9, "linear", "planar", seed=35)
    line("K17 tm_stack_certify three windows", *st.certify(bent_cuts(33, 33, 2), highorder.Elevation(1, "gauss_lobatto"), 0, max_depth=2))
    del os.environ["TM_HO3_CERT_WINDOW_BYTES"]


def weld_stages():
    for name in ("two_by_two_junction", "channel_periodic_sliding", "strip3_reversed", "plate_le"):
        mesh = TOPOLOGIES[name](None)
        wd = weld.Weld(mesh)
        line(f"K18 tm_weld_map {name}", wd.map, wd.info)
        pts = wd.points(mesh)
        line(f"K18 tm_weld_points {name}", pts, wd.info)
        line(f"K18 tm_weld_cells {name}", wd.cells(1))
        b = wd.boundary(1)
        line(f"K19 tm_weld_boundary_faces {name}", b.faces, b.face_patch, b.origin)
        line(f"K19 tm_weld_faces_measure {name}", b.measure(pts))
        with smooth.Smoother(mesh, RELAX) as sm:
            sm.iterate(2)
            um = sm.weld()
            line(f"K18 tm_smoother_weld {name}", um.points, um.cells)
            line(f"K19 tm_smoother_weld_boundary {name}", *sm.weld_boundary(1))
    mesh = configs.two_by_two(9, 9)
    hom = highorder.Elevation(2, "gauss_lobatto").mesh(mesh)
    wd = weld.Weld(mesh)
    line("K18 welded K13 planes", wd.points(hom), wd.info, wd.cells(2))
    blocks = [tuple(np.stack([pl * (1.0 + k / 3.0) if c < 2 else pl + k / 7.0 for k in range(3)]) for c, pl in enumerate((m.points.data[..., 0].T.copy(), m.points.data[..., 1].T.copy(),
                                                                                                                     np.zeros(m.points.size[::-1]))))
              for m in mesh.blocks]
    line("K18 hexahedra on three layers", wd.points(blocks), wd.cells(2, 3))
    b = wd.boundary(2, 3)
    line("K19 faces on three layers", b.faces, b.face_patch, b.origin, b.measure(wd.points(blocks)))
    with smooth.Smoother(configs.two_by_two(33, 33), RELAX) as sm:
        error("K19 no elements of order 3", lambda: sm.weld_boundary(3))


def csr_stages():
    # the solver slot and the handle's assembled modes keep their vectors in the same device buffers
    n = 200
    Ap = np.concatenate([[0], np.cumsum([2] + [3] * (n - 2) + [2])]).astype(np.int32)
    Ai = np.concatenate([[0, 1]] + [[i - 1, i, i + 1] for i in range(1, n - 1)] + [[n - 2, n - 1]]).astype(np.int32)
    Ax = np.concatenate([[2.0, -1.0]] + [[-1.0, 2.0, -1.0]] * (n - 2) + [[-1.0, 2.0]])
    b = np.sin(np.arange(n) * 0.37)
    b2 = 2.0 * b
    lu, z = np.empty(len(Ax)), np.empty(n)
    _capi.check(_capi.lib().tm_csr_ilu0_probe(n, Ap.ctypes.data_as(_ip), Ai.ctypes.data_as(_ip), _capi.f64ptr(Ax), _capi.f64ptr(b), _capi.f64ptr(lu), _capi.f64ptr(z)))
    line("csr tm_csr_ilu0_probe", lu, z)
    for name, opt in (("bicgstab", dict()), ("bicgstab_ilu0", dict(preconditioner=solver.Preconditioner.ilu0)),
                      ("gmres_ilu0", dict(inner=solver.Inner.reference_gmres, preconditioner=solver.Preconditioner.ilu0))):
        x, y = np.zeros(n), np.zeros(n)
        o = solver.Option.hip(rtol=1e-12, max_inner=400, check_every=1, **opt).c_struct()
        st = _capi.tm_stats()
        rc = _capi.lib().tm_csr_solve(n, Ap.ctypes.data_as(_ip), Ai.ctypes.data_as(_ip), _capi.f64ptr(Ax), None, _capi.f64ptr(b), _capi.f64ptr(b2), _capi.f64ptr(x),
                                      _capi.f64ptr(y), C.byref(o), C.byref(st))
        line(f"csr tm_csr_solve {name} rc {rc}", x, y)
    for mode in (dict(inner=solver.Inner.reference_gmres), dict(inner=solver.Inner.reference_gmres, preconditioner=solver.Preconditioner.ilu0)):
        mesh = TOPOLOGIES["two_by_two_junction"](None)
        with smooth.Smoother(mesh, solver.Option.hip(**mode)) as sm:
            sm.iterate(2)
            sm.download()
        line(f"handle reference_gmres {sorted(mode)}", *[blk.points.data for blk in mesh.blocks])
    e = configs.single_block_edges(33, 41)
    line("tm_tfi_block 33x41", Block2d.init(*e).points.data)


if __name__ == "__main__":
    for stage in (quality_stage, stack_stages, flat_highorder, stacked_highorder, weld_stages, csr_stages):
        stage()
