"""CPU: spanwise stacking (include/tm_hip.h, "3-D from 2-D cuts") without a GPU -- tm_stack_weights and tm_stack_block_host against the
longdouble reference written from the definition (tests/stack_reference.py), the error codes, the 3-D PLOT3D file, the CLI's argument
errors.  eps = 2^-52 throughout; every bar is the issue's."""
import ctypes as C

import numpy as np
import pytest

from tests import control_field_reference as cfr
from tests import stack_reference as sr
from turbomesh_amd import _capi, output, stack

EPS = sr.EPS
LD = np.longdouble


def cut_meshes(blocks):
    return [cfr.single_block_mesh(b) for b in blocks]


def bent_cuts(ni, nj, K):
    """The cuts of the device tests: bent_clustered with seed c, shifted by 0.01 c."""
    return [cfr.bent_clustered(ni, nj, seed=c) + 0.01 * c for c in range(K)]


# ------------------------------------------------------------------ weights
@pytest.mark.parametrize("K", [2, 3, 5, 16])
@pytest.mark.parametrize("kind", ["uniform", "nonuniform"])
@pytest.mark.parametrize("interpolation", ["linear", "cubic"])
def test_weights_against_reference(K, kind, interpolation):
    z = sr.spans(K, kind)
    s = sr.layers_with_cuts(z, 33, seed=K)
    assert all(np.any(s == zc) for zc in z)   # 33 points including every cut
    A = stack.Stack(z, s, interpolation).weights()
    ref = sr.weights_ref(z, s, interpolation)
    assert A.shape == ref.shape == (33, K)
    bar = 4 * EPS * np.abs(ref).sum(axis=1, keepdims=True)
    ratio = float(np.max(np.abs(A.astype(LD) - ref) / bar))
    print(f"stack_parity: weights K={K} {kind} {interpolation}: worst |A - A_ref| / bar = {ratio:.3f}")
    assert ratio <= 1.0
    # rows at cuts are exactly e_c
    for k, sk in enumerate(s):
        hit = np.nonzero(z == sk)[0]
        if hit.size:
            assert np.array_equal(A[k], np.eye(K)[hit[0]])
    # rows sum to 1
    assert np.all(np.abs(A.astype(LD).sum(axis=1) - 1) <= 4 * EPS * np.abs(A).sum(axis=1))


def test_cubic_with_two_cuts_is_linear_bit_for_bit():
    z = np.array([0.3, 1.7])
    s = sr.layers_with_cuts(z, 33)
    assert np.array_equal(stack.Stack(z, s, "cubic").weights(), stack.Stack(z, s, "linear").weights())


def test_linear_weights_are_the_two_neighbours():
    z = sr.spans(5, "nonuniform")
    s = np.array([0.5 * (z[2] + z[3])])
    A = stack.Stack(z, s, "linear").weights()
    assert np.count_nonzero(A) == 2 and A[0, 2] == 0.5 and A[0, 3] == 0.5


# ------------------------------------------------------------------ values on the host
@pytest.mark.parametrize("K,kind", [(2, "uniform"), (3, "nonuniform"), (5, "uniform"), (16, "nonuniform")])
@pytest.mark.parametrize("interpolation", ["linear", "cubic"])
def test_affine_in_span_is_reproduced(K, kind, interpolation):
    # v_c = p + z_c q node-wise: both interpolations reproduce p + s_k q
    z = sr.spans(K, kind)
    s = sr.layers_with_cuts(z, 9, seed=3)
    p, q = cfr.bent_clustered(7, 6).astype(LD), (cfr.bent_clustered(7, 6, seed=2) - 0.4).astype(LD)
    blocks = [np.asarray(p + LD(zc) * q, dtype=np.float64) for zc in z]
    st = stack.Stack(z, s, interpolation)
    X, Y, Z = st.block(cut_meshes(blocks), 0, host=True)
    A = st.weights()
    bx, by, _ = sr.stack_bar(blocks, A, "planar", z, s)
    want = p[None] + s.astype(LD)[:, None, None, None] * q[None]   # (nk, ni, nj, 2)
    rx = sr.worst_ratio(X, np.transpose(want[..., 0], (0, 2, 1)), bx)
    ry = sr.worst_ratio(Y, np.transpose(want[..., 1], (0, 2, 1)), by)
    print(f"stack_parity: affine K={K} {kind} {interpolation}: worst ratio x {rx:.3f} y {ry:.3f}")
    assert rx <= 1.0 and ry <= 1.0
    assert np.array_equal(Z, np.broadcast_to(s[:, None, None], Z.shape))


@pytest.mark.parametrize("K,kind,interpolation,mapping", [
    (2, "uniform", "cubic", "planar"), (3, "nonuniform", "cubic", "cylindrical"), (5, "nonuniform", "linear", "cylindrical"),
    (16, "uniform", "cubic", "cylindrical"), (16, "nonuniform", "cubic", "planar"), (5, "uniform", "linear", "planar"),
])
def test_host_values_within_the_dot_product_bound(K, kind, interpolation, mapping):
    z = sr.spans(K, kind)
    s = sr.layers_with_cuts(z, 7, seed=K)
    blocks = bent_cuts(9, 11, K)
    st = stack.Stack(z, s, interpolation, mapping)
    got = st.block(cut_meshes(blocks), 0, host=True)
    A = st.weights()   # the library's own weights: their error is judged above
    ref = sr.stack_ref(blocks, A, mapping, z, s)
    bar = sr.stack_bar(blocks, A, mapping, z, s)
    ratios = [sr.worst_ratio(g, r, b) if np.any(b > 0) else float(np.max(np.abs(g.astype(LD) - r))) for g, r, b in zip(got, ref, bar)]
    print(f"stack_parity: host K={K} {kind} {interpolation} {mapping}: worst ratio x {ratios[0]:.3f} y {ratios[1]:.3f} z {ratios[2]:.3f}")
    assert max(ratios) <= 1.0
    if mapping == "planar":
        assert np.array_equal(got[2], np.broadcast_to(s[:, None, None], got[2].shape))
        for k, sk in enumerate(s):   # a layer at a cut reproduces the cut
            hit = np.nonzero(z == sk)[0]
            if hit.size:
                assert np.array_equal(got[0][k], blocks[hit[0]][..., 0].T) and np.array_equal(got[1][k], blocks[hit[0]][..., 1].T)


def test_windows_concatenate_on_the_host():
    z, K = sr.spans(3, "nonuniform"), 3
    s = sr.layers_with_cuts(z, 7)
    st = stack.Stack(z, s)
    cuts = cut_meshes(bent_cuts(5, 4, K))
    full = st.block(cuts, 0, host=True)
    a, b = st.block(cuts, 0, 0, 3, host=True), st.block(cuts, 0, 3, host=True)
    for f, p, q in zip(full, a, b):
        assert f.shape == (7, 4, 5) and np.array_equal(f, np.concatenate([p, q]))


# ------------------------------------------------------------------ errors
def _call_host(span, layers, cuts, block=0, k_begin=0, k_count=None, interpolation=1, mapping=0, null=None):
    span, layers = np.asarray(span, dtype=np.float64), np.asarray(layers, dtype=np.float64)
    opt = _capi.tm_stack_opt(span.size, _capi.f64ptr(span), layers.size, _capi.f64ptr(layers), interpolation, mapping)
    descs = [_capi.MeshDesc(m) for m in cuts]
    arr = (C.POINTER(_capi.tm_mesh_desc) * max(1, len(descs)))(*[C.pointer(d.desc) for d in descs])
    k_count = layers.size - k_begin if k_count is None else k_count
    ni, nj = cuts[0].blocks[0].points.size
    out = [np.empty(max(1, k_count) * ni * nj) for _ in range(3)]
    ptrs = [None if null == f"out{q}" else _capi.f64ptr(out[q]) for q in range(3)]
    return _capi.lib().tm_stack_block_host(None if null == "cuts" else arr, None if null == "opt" else C.byref(opt), block, k_begin, k_count, *ptrs)


def test_argument_errors():
    cuts3 = cut_meshes(bent_cuts(4, 5, 3))
    ok = dict(span=[1.0, 2.0, 3.0], layers=[1.0, 1.5, 3.0], cuts=cuts3)
    assert _call_host(**ok) == _capi.TM_OK
    E = _capi.TM_E_ARG
    assert _call_host(**{**ok, "span": [1.0, 1.0, 3.0]}) == E            # not strictly increasing
    assert _call_host(**{**ok, "span": [1.0, 3.0, 2.0]}) == E
    assert _call_host(**{**ok, "span": [1.0, np.nan, 3.0]}) == E
    assert _call_host(**{**ok, "layers": [1.0, 3.0000001]}) == E         # a layer outside the span: no extrapolation
    assert _call_host(**{**ok, "layers": [0.999, 2.0]}) == E
    assert _call_host(**{**ok, "layers": [1.0, np.inf]}) == E
    assert _call_host(span=[1.0], layers=[1.0], cuts=cuts3[:1]) == E      # K = 1
    z17 = np.arange(17) + 1.0
    assert _call_host(span=z17, layers=[1.0], cuts=cut_meshes(bent_cuts(3, 3, 17))) == E   # K = 17
    assert _call_host(**{**ok, "layers": []}) == E                       # nk = 0
    assert _call_host(**{**ok, "span": [0.0, 2.0, 3.0], "layers": [2.0], "mapping": 1}) == E   # z <= 0 with the cylindrical mapping
    assert _call_host(**{**ok, "span": [-1.0, 2.0, 3.0], "layers": [2.0], "mapping": 1}) == E
    assert _call_host(**{**ok, "span": [0.0, 2.0, 3.0], "layers": [2.0], "mapping": 0}) == _capi.TM_OK
    assert _call_host(**{**ok, "k_begin": 1, "k_count": 3}) == E         # a window past nk
    assert _call_host(**{**ok, "k_begin": 3, "k_count": 1}) == E
    assert _call_host(**{**ok, "k_begin": 0, "k_count": 0}) == E
    assert _call_host(**{**ok, "block": 1}) == E
    assert _call_host(**{**ok, "interpolation": 7}) == E
    assert _call_host(**{**ok, "mapping": 7}) == E
    for null in ("cuts", "opt", "out0", "out1", "out2"):
        assert _call_host(**{**ok, "null": null}) == E
    assert b"" != _capi.lib().tm_last_error()
    # weights: the same validation, and a NULL output
    span, layers = np.array([1.0, 2.0]), np.array([1.5])
    opt = _capi.tm_stack_opt(2, _capi.f64ptr(span), 1, _capi.f64ptr(layers), 1, 0)
    assert _capi.lib().tm_stack_weights(C.byref(opt), None) == E
    assert _capi.lib().tm_stack_weights(None, _capi.f64ptr(np.empty(2))) == E
    opt.span = None
    assert _capi.lib().tm_stack_weights(C.byref(opt), _capi.f64ptr(np.empty(2))) == E


def test_size_errors():
    ok = cut_meshes(bent_cuts(4, 5, 3))
    z, s = [1.0, 2.0, 3.0], [1.5]
    other = cut_meshes([cfr.bent_clustered(4, 6)])[0]                     # the block differs in nj
    assert _call_host(z, s, [ok[0], other, ok[2]]) == _capi.TM_E_SIZE
    two = cfr.single_block_mesh(cfr.bent_clustered(4, 5))
    from turbomesh_amd import configs

    two.addBlock("block_1", configs.block_from_array(cfr.bent_clustered(4, 5, seed=1)))   # the cuts differ in block count
    assert _call_host(z, s, [ok[0], ok[1], two]) == _capi.TM_E_SIZE
    with pytest.raises(_capi.TmError) as e:
        stack.Stack(z, s).block([ok[0], other, ok[2]], 0, host=True)
    assert e.value.code == _capi.TM_E_SIZE
    with pytest.raises(ValueError):
        stack.Stack(z, s).block(ok[:2], 0, host=True)                     # two cuts for three span positions


# ------------------------------------------------------------------ layers, file format, CLI
def test_layers_from():
    from turbomesh_amd import clustering

    z = [0.25, 0.5, 1.75]
    s = stack.layers_from(z, 5)
    assert s[0] == 0.25 and s[-1] == 1.75 and np.allclose(s, np.linspace(0.25, 1.75, 5), rtol=0, atol=1e-15)
    t = stack.layers_from(z, 9, clustering.SingleHyperbolicClustering(0.02))
    assert t[0] == 0.25 and t[-1] == 1.75 and np.all(np.diff(t) > 0)
    u = clustering.create(clustering.SingleHyperbolicClustering(0.02), 9)
    assert np.allclose(t, 0.25 + u * 1.5, rtol=0, atol=1e-15)
    assert np.array_equal(stack.layers_from(z, 1), [0.25])
    with pytest.raises(ValueError):
        stack.layers_from(z, 0)
    with pytest.raises(ValueError):
        stack.Stack(z, s, interpolation="quintic")


def test_plot3d_3d_round_trip_is_bit_exact(tmp_path):
    rng = np.random.default_rng(5)
    sizes = [(5, 4, 3), (2, 7, 1)]
    planes = [tuple(rng.standard_normal((nk, nj, ni)) for _ in range(3)) for ni, nj, nk in sizes]
    f = str(tmp_path / "m.xyz")
    output.write_plot3d_3d(f, sizes, planes)
    raw = np.fromfile(f, dtype="<i4", count=7)
    assert list(raw) == [2, 5, 4, 3, 2, 7, 1]
    import os

    assert os.path.getsize(f) == 4 * 7 + 8 * 3 * (60 + 14)
    back = output.read_plot3d_3d(f)
    assert [(b[0], b[1], b[2]) for b in back] == sizes
    for (ni, nj, nk, X, Y, Z), (x, y, z) in zip(back, planes):
        assert np.array_equal(X, x) and np.array_equal(Y, y) and np.array_equal(Z, z)
    # i fastest: the first doubles of block 0 are x[k=0, j=0, i=0..4]
    first = np.fromfile(f, dtype="<f8", count=5, offset=28)
    assert np.array_equal(first, planes[0][0][0, 0, :])
    # Mesh3d writes the same file
    g = str(tmp_path / "n.p3d")
    stack.Mesh3d(["a", "b"], planes).write(g)
    assert open(f, "rb").read() == open(g, "rb").read()
    with pytest.raises(output.OutputFormatNotEnabled):
        stack.Mesh3d(["a", "b"], planes).write(str(tmp_path / "n.cgns"))


@pytest.mark.parametrize("argv,message", [
    (["a.json", "--hip", "--stack", "b.json", "c.json", "--span", "0,1", "--layers", "5", "--output", "o.xyz"], "--span has 2 values for 3 files"),
    (["a.json", "--hip", "--stack", "b.json", "--layers", "5", "--output", "o.xyz"], "--stack needs --span"),
    (["a.json", "--hip", "--stack", "b.json", "--span", "0,1", "--output", "o.xyz"], "--stack needs --span"),
    (["a.json", "--hip", "--stack", "b.json", "--span", "0,x", "--layers", "5", "--output", "o.xyz"], "comma-separated numbers"),
    (["a.json", "--hip", "--stack", "b.json", "--span", "0,1", "--layers", "5"], "--stack needs --output"),
    (["a.json", "--hip", "--stack", "b.json", "--span", "0,1", "--layers", "5", "--output", "o.xyz", "--span-clustering", "roberts:1"], "--span-clustering"),
    (["a.json", "--hip", "--span", "0,1"], "go with --stack"),
])
def test_cli_argument_errors(capsys, argv, message):
    from turbomesh_amd.__main__ import main

    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err
