"""GPU tests of ScalableTSDFVolume.extract_triangle_mesh (csrc/tsdf.hip, marching cubes on the device) against the numpy
restatement tests/tsdf_mesh_ref.py on the states of tests/tsdf_mesh_cases.py, loaded through load_units.  Everywhere: the counts
equal, vertices and colours bit for bit (sums, products and quotients of float64 in a fixed order), triangles entry by entry,
every index inside [0, nv) and every vertex used.  The restatement's meshes are computed once per session and left unchanged."""
import ctypes

import numpy as np
import pytest

from tests import tsdf_mesh_cases as mc
from tests import tsdf_mesh_ref as mr

pytestmark = pytest.mark.gpu


def _volume(r3d, color=True, initial_units=4, ctx=None):
    kind = r3d.TSDFVolumeColorType.RGB8 if color else r3d.TSDFVolumeColorType.NoColor
    return r3d.ScalableTSDFVolume(mc.VL, mc.TRUNC, kind, initial_units=initial_units, ctx=ctx)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check(mesh, want, what):
    vert, col, tri = want
    assert (len(mesh.vertices), len(mesh.triangles)) == (len(vert), len(tri)), f"{what}: counts {len(mesh.vertices)}, {len(mesh.triangles)}"
    assert mesh.vertices.dtype == np.float64 and mesh.triangles.dtype == np.int32 and mesh.vertex_normals is None
    bad = (_bits(mesh.vertices) != _bits(vert)).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} vertices differ in their bits, first {int(np.argmax(bad))}"
    if col is None:
        assert mesh.vertex_colors is None and not mesh.has_vertex_colors()
    else:
        bad = (_bits(mesh.vertex_colors) != _bits(col)).any(1)
        assert not bad.any(), f"{what}: {int(bad.sum())} colours differ in their bits, first {int(np.argmax(bad))}"
    bad = (mesh.triangles != tri).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} triangles differ, first {int(np.argmax(bad))}"
    if len(tri):
        assert mesh.triangles.min() >= 0 and mesh.triangles.max() < len(vert)
        assert len(np.unique(mesh.triangles)) == len(vert), f"{what}: a vertex no triangle uses"


def _loaded(r3d, name, color=True, initial_units=4, ctx=None):
    state = mc.CASES[name]()
    volume = _volume(r3d, color, initial_units, ctx)
    volume.load_units(*(state if color else mc.without_colour(state)))
    return volume


def _state_bytes(volume):
    return [None if a is None else a.tobytes() for a in volume.debug_units()]


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [True, False])
def test_all_256_configurations(r3d, color):
    want = mc.reference("configurations", color)
    table = r3d.tsdf.mc_table()
    with _loaded(r3d, "configurations", color) as volume:
        assert len(volume) == 4 and volume.mesh_counts() == mc.COUNTS["configurations"]
        mesh = volume.extract_triangle_mesh()
        _check(mesh, want, "configurations")
        base = np.floor(mesh.vertices[mesh.triangles[:, 0]] / mc.VL - 0.5 + 1e-9).astype(int)
        block = (base[:, 0] + 16) // 3 + 8 * ((base[:, 1] + 16) // 3) + 64 * (base[:, 2] // 3)
        assert np.array_equal(np.bincount(block, minlength=256), (table >= 0).sum(1) // 3), "a block's triangle count is not its row's"


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
def test_closed_surface_across_eight_units(r3d):
    with _loaded(r3d, "sphere") as volume:
        mesh = volume.extract_triangle_mesh()
    _check(mesh, mc.reference("sphere"), "sphere")
    repeated, boundary, undirected = mr.edge_census(mesh.triangles)
    assert repeated == 0 and boundary == 0, "the surface is not closed or not consistently oriented"
    assert len(mesh.vertices) - undirected + len(mesh.triangles) == 2
    ratio = mr.signed_volume(mesh.vertices, mesh.triangles) / (4.0 / 3.0 * np.pi * mc.SPHERE_R ** 3)
    print(f"sphere: {len(mesh.vertices)} vertices, {len(mesh.triangles)} triangles, volume ratio {ratio:.4f}")
    assert 0.9 < ratio < 1.0
    mesh.compute_vertex_normals()
    n = mesh.vertex_normals
    assert mesh.has_vertex_normals() and np.abs(np.sqrt((n * n).sum(1)) - 1.0).max() < 1e-12
    assert ((n * (mesh.vertices - mc.SPHERE_C)).sum(1) > 0).all(), "a vertex normal looks inward"


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,is_open", [("no_unit_000", True), ("no_unit_mmm", True), ("corner_voxel", False), ("through_corner", True)])
def test_holes_and_absent_units(r3d, name, is_open):
    with _loaded(r3d, name) as volume:
        mesh = volume.extract_triangle_mesh()
    _check(mesh, mc.reference(name), name)
    repeated, boundary, _ = mr.edge_census(mesh.triangles)
    assert repeated == 0 and (boundary > 0) == is_open


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
def test_more_than_256_units(r3d):
    want = mc.reference("plane")
    outs = []
    for initial in (1, 600):
        with _loaded(r3d, "plane", initial_units=initial) as volume:
            assert len(volume) == 300 and volume.stats()["capacity"] == max(initial, 300)
            mesh = volume.extract_triangle_mesh()
            outs.append((mesh.vertices.tobytes(), mesh.vertex_colors.tobytes(), mesh.triangles.tobytes()))
            if initial == 1:
                _check(mesh, want, "plane")
                idx = volume.debug_units()[0]
                assert np.array_equal(idx, np.array(sorted(map(tuple, mc.plane()[0])), np.int32))
    assert outs[0] == outs[1]
    with _loaded(r3d, "plane", color=False, initial_units=1) as volume:
        _check(volume.extract_triangle_mesh(), mc.reference("plane", False), "plane without colour")


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------
def test_index_limits(r3d):
    with _loaded(r3d, "limits") as volume:
        mesh = volume.extract_triangle_mesh()
        _check(mesh, mc.reference("limits"), "limits")
        assert np.abs(mesh.vertices).max() > (mc.LIMIT - 1) * 16 * mc.VL


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------
def test_integrated_state(r3d):
    from tests import rgbd_scene as sc
    from tests import test_tsdf_gpu as tg
    want = mc.reference("integrated")
    cam = sc.camera(64, 48)
    with tg._volume(r3d) as volume, _volume(r3d, initial_units=8) as copy:
        for k, pose in enumerate(tg.POSES_A):
            depth, color = tg._frame(64, 48, k)
            volume.integrate_f32(depth, color, cam, np.linalg.inv(pose))
        state = volume.debug_units()
        cloud_before = [a.tobytes() for a in volume.extract_arrays()]
        mesh = volume.extract_triangle_mesh()
        assert [a.tobytes() for a in state] == [a.tobytes() for a in mc.integrated()]      # so `want` is the restatement of debug_units()
        _check(mesh, want, "case A")
        assert [a.tobytes() for a in volume.extract_arrays()] == cloud_before, "a mesh extraction changed the cloud"
        assert _state_bytes(volume) == [a.tobytes() for a in state]
        copy.load_units(*state)
        assert _state_bytes(copy) == [a.tobytes() for a in state] and copy.stats()["frames"] == 0 and volume.stats()["frames"] == 3
        again = copy.extract_triangle_mesh()
        assert (again.vertices.tobytes(), again.vertex_colors.tobytes(), again.triangles.tobytes()) == \
            (mesh.vertices.tobytes(), mesh.vertex_colors.tobytes(), mesh.triangles.tobytes())
        assert [a.tobytes() for a in copy.extract_arrays()] == cloud_before
    frames = []
    for k in range(3):
        depth, color = tg._frame(64, 48, k)
        frames.append((color, np.round(depth * 1000.0).astype(np.uint16)))
    camera = r3d.cloud_ops.depth_camera(dict(fx=cam[0], fy=cam[1], ppx=cam[2], ppy=cam[3]), depth_scale=1000.0, depth_trunc=3.0)
    fused = r3d.pipeline.tsdf_fuse(frames, camera, list(tg.POSES_A), tg.VL, tg.TRUNC, color=True, initial_units=8, mesh=True)
    assert isinstance(fused, r3d.TriangleMesh) and fused.has_triangles() and fused.has_vertex_colors()
    with tg._volume(r3d) as volume:
        for (color, raw), pose in zip(frames, tg.POSES_A):
            volume.integrate(r3d.cloud_ops.rgbd_image(color, raw, 1000.0, 3.0), cam, np.linalg.inv(pose))
        direct = volume.extract_triangle_mesh()
    assert (fused.vertices.tobytes(), fused.vertex_colors.tobytes(), fused.triangles.tobytes()) == \
        (direct.vertices.tobytes(), direct.vertex_colors.tobytes(), direct.triangles.tobytes())
    assert isinstance(r3d.pipeline.tsdf_fuse(frames, camera, list(tg.POSES_A), tg.VL, tg.TRUNC, initial_units=8), r3d.PointCloud)


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------
def _code(fn, *args):
    with pytest.raises(Exception) as e:
        fn(*args)
    assert hasattr(e.value, "code") and str(e.value).split(":", 1)[1].strip(), "no message came through r3d_last_error"
    return e.value.code


def test_interface(r3d, tmp_path):
    start = r3d._lib.live_resources()
    ctx = r3d.Context(0)                 # a context of its own: its arena goes with it
    want = mc.reference("sphere")
    nv, nt = len(want[0]), len(want[2])
    volume = _loaded(r3d, "sphere", ctx=ctx)
    assert volume.mesh_counts() == (nv, nt)
    first = volume.extract_triangle_mesh()
    second = volume.extract_triangle_mesh()
    assert (first.vertices.tobytes(), first.vertex_colors.tobytes(), first.triangles.tobytes()) == \
        (second.vertices.tobytes(), second.vertex_colors.tobytes(), second.triangles.tobytes())
    # a capacity one short: R3D_E_BADARG, the counts returned, nothing written
    for cap_v, cap_t in ((nv - 1, nt), (nv, nt - 1), (nv, 0), (0, nt)):
        vert, col, tri = np.full((nv, 3), 7.0), np.full((nv, 3), 7.0), np.full((nt, 3), 7, np.int32)
        gv, gt = ctypes.c_int64(), ctypes.c_int64()
        ptr = [a.ctypes.data_as(ctypes.c_void_p) for a in (vert, col, tri)]
        assert _code(ctx.call, "r3d_mesh_from_volume", volume._h, cap_v, cap_t, *ptr, ctypes.byref(gv), ctypes.byref(gt)) == -1
        assert (gv.value, gt.value) == (nv, nt) and (vert == 7.0).all() and (col == 7.0).all() and (tri == 7).all(), "a refused extraction wrote"
    gv, gt = ctypes.c_int64(), ctypes.c_int64()
    assert _code(ctx.call, "r3d_mesh_from_volume", volume._h, nv, nt, ptr[0], None, ptr[2], ctypes.byref(gv), ctypes.byref(gt)) == -1     # RGB8 without colours
    assert _code(ctx.call, "r3d_mesh_from_volume", volume._h, nv, nt, ptr[0], ptr[1], None, ctypes.byref(gv), ctypes.byref(gt)) == -1
    assert _code(ctx.call, "r3d_mesh_from_volume", volume._h, -1, nt, *ptr, ctypes.byref(gv), ctypes.byref(gt)) == -1
    assert _code(ctx.call, "r3d_mesh_from_volume", volume._h, nv, nt, *ptr, None, ctypes.byref(gt)) == -1
    # the device form, with room to spare and a sentinel behind the rows
    d_vert, d_col, d_tri = ctx.to_device(np.full((nv + 1, 3), 7.0)), ctx.to_device(np.full((nv + 1, 3), 7.0)), ctx.to_device(np.full((nt + 1, 3), 7, np.int32))
    try:
        assert volume.extract_mesh_device(d_vert, d_col, d_tri, nv + 1, nt + 1) == (nv, nt)
        vert, col, tri = np.empty((nv + 1, 3)), np.empty((nv + 1, 3)), np.empty((nt + 1, 3), np.int32)
        for host, dev in ((vert, d_vert), (col, d_col), (tri, d_tri)):
            ctx.d2h(host, dev)
        assert vert[:nv].tobytes() == first.vertices.tobytes() and col[:nv].tobytes() == first.vertex_colors.tobytes()
        assert tri[:nt].tobytes() == first.triangles.tobytes()
        assert (vert[nv] == 7.0).all() and (col[nv] == 7.0).all() and (tri[nt] == 7).all()
    finally:
        for d in (d_vert, d_col, d_tri):
            ctx.free(d)
    # load_units refusals leave the volume as it was
    before = _state_bytes(volume)
    idx, tsdf, weight, colour = mc.sphere()
    twice = idx.copy()
    twice[5] = twice[2]
    assert _code(volume.load_units, twice, tsdf, weight, colour) == -1
    for bad in (mc.LIMIT, -mc.LIMIT - 1):
        far = idx.copy()
        far[7, 1] = bad
        assert _code(volume.load_units, far, tsdf, weight, colour) == -1
    assert _code(ctx.call, "r3d_debug_volume_load_units", volume._h, 8, None, None, None, None) == -1
    assert _state_bytes(volume) == before and volume.mesh_counts() == (nv, nt)
    # fewer units than before, then none, then a reset volume
    volume.load_units(idx[:3], tsdf[:3], weight[:3], colour[:3])
    assert len(volume) == 3 and np.array_equal(volume.debug_units()[0], idx[:3])
    three = volume.extract_triangle_mesh()
    _check(three, mr.mesh(idx[:3], tsdf[:3], weight[:3], colour[:3], mc.VL, r3d.tsdf.mc_table()), "three units")
    volume.load_units(np.zeros((0, 3), np.int32), np.zeros((0, 4096), np.float32), np.zeros((0, 4096), np.float32), np.zeros((0, 3, 4096)))
    assert len(volume) == 0 and volume.mesh_counts() == (0, 0)
    volume.load_units(idx, tsdf, weight, colour)
    assert volume.mesh_counts() == (nv, nt)
    volume.reset()
    assert volume.mesh_counts() == (0, 0)
    empty = volume.extract_triangle_mesh()
    assert empty.vertices.shape == (0, 3) and empty.triangles.shape == (0, 3) and not empty.has_triangles() and not empty.has_vertices()
    volume.close()
    with _volume(r3d, ctx=ctx) as fresh:
        assert fresh.mesh_counts() == (0, 0)
    with _loaded(r3d, "sphere", color=False, ctx=ctx) as grey:
        mesh = grey.extract_triangle_mesh()
        assert mesh.vertex_colors is None and mesh.vertices.tobytes() == first.vertices.tobytes() and mesh.triangles.tobytes() == first.triangles.tobytes()
    ctx.close()
    assert r3d._lib.live_resources() == start, "a volume or a mesh extraction left GPU resources behind"
    # hand-off to the PLY writer
    path = str(tmp_path / "mesh.ply")
    r3d.io_formats.write_ply(path, first.vertices, colors=first.vertex_colors, faces=first.triangles)
    back = r3d.io_formats.read_ply(path)
    assert np.array_equal(back["faces"], first.triangles) and len(back["points"]) == nv
    moved = r3d.TriangleMesh(first.vertices.copy(), first.triangles).transform(np.array([[1, 0, 0, 1.0], [0, 1, 0, 2.0], [0, 0, 1, 3.0], [0, 0, 0, 1]]))
    assert np.abs(moved.vertices - (first.vertices + (1.0, 2.0, 3.0))).max() < 1e-12
