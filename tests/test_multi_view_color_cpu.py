"""Colours through the multi-view fusion (BASELINE config C5), without a GPU: the HIP registration and transform are replaced
by injected stubs, as in tests/test_distributed_cpu.py; one rank needs no process group.  What is checked is the plumbing the
GPUs run too: colours travel as a third plane, are never moved by a rigid transform, and come out in view order."""
import numpy as np
import pytest


def _clouds(r3d, n_views, colored):
    """view v = the same planar patch displaced by a known translation, 40 + 3 v points; `colored`: the views that get colours"""
    rng = np.random.default_rng(11)
    base = np.concatenate([rng.random((60, 2)), np.zeros((60, 1))], 1)
    shifts = {v: np.array([0.01 * v, -0.02 * v, 0.005 * v]) for v in range(n_views)}
    clouds = {}
    for v in range(n_views):
        n = 40 + 3 * v
        clouds[v] = r3d.PointCloud(base[:n] - shifts[v], colors=rng.random((n, 3)) if v in colored else None,
                                   normals=np.tile([0, 0, 1.0], (n, 1)))
    return clouds, base, shifts


def _stub_register(src, tgt):                       # exact for pure translations of the same leading points
    assert src.ndim == 2 and src.shape[1] == 6 and tgt.shape[1] == 6          # rows stay xyz | normal: colours are not shown
    T = np.eye(4)
    T[:3, 3] = tgt[:40, :3].mean(0) - src[:40, :3].mean(0)
    return T


@pytest.fixture()
def host_exchange(monkeypatch):
    """the exchange on host tensors, whether or not this machine has a GPU (the stubs do the device work)"""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_fused_cloud_keeps_the_colours_in_view_order(r3d, host_exchange):
    clouds, base, shifts = _clouds(r3d, 3, colored={0, 1, 2})
    fused, Ts = r3d.pipeline.multi_view_fuse(clouds, 3, register=_stub_register)
    assert fused.has_colors() and fused.has_normals() and len(fused) == sum(len(c) for c in clouds.values())
    np.testing.assert_array_equal(fused.colors, np.concatenate([clouds[v].colors for v in range(3)]))
    for v in range(3):
        assert np.abs(Ts[v][:3, 3] - shifts[v]).max() < 1e-12
    assert np.abs(fused.points[:40] - base[:40]).max() < 1e-12 and np.abs(fused.points[40:80] - base[:40]).max() < 1e-12


def test_mixed_coloured_and_colourless_clouds_are_refused(r3d, host_exchange):
    clouds, _, _ = _clouds(r3d, 3, colored={0, 2})
    with pytest.raises(ValueError, match=r"\[2, n, 3\].*\[3, n, 3\]"):
        r3d.pipeline.multi_view_fuse(clouds, 3, register=_stub_register)


def test_colourless_clouds_still_fuse_without_colours(r3d, host_exchange):
    clouds, base, _ = _clouds(r3d, 3, colored=set())
    fused, _ = r3d.pipeline.multi_view_fuse(clouds, 3, register=_stub_register)
    assert not fused.has_colors() and fused.colors.shape == (0, 3) and fused.has_normals()
    assert np.abs(fused.points[:40] - base[:40]).max() < 1e-12


def test_three_plane_tensors_leave_plane_two_untouched(r3d, host_exchange):
    import torch
    rng = np.random.default_rng(3)
    local = {v: torch.from_numpy(rng.random((3, 5 + v, 3))) for v in range(3)}
    seen = []

    def register(src, tgt):
        seen.append((tuple(src.shape), tuple(tgt.shape)))
        T = np.eye(4)
        T[:3, 3] = 0.5
        return T

    def transform(blk, T):                          # moves EVERY plane it is given: plane 2 must not be among them
        assert blk.shape[0] == 2
        return blk + float(T[0, 3])
    fused, Ts = r3d.pipeline.multi_view_fuse_tensors(local, 3, register=register, transform=transform)
    assert fused.shape == (3, 5 + 6 + 7, 3) and seen == [((2, 6, 3), (2, 5, 3)), ((2, 7, 3), (2, 5, 3))]
    assert torch.equal(fused[2], torch.cat([local[v][2] for v in range(3)]))
    assert torch.equal(fused[:2, :5], local[0][:2]) and torch.equal(fused[:2, 5:11], local[1][:2] + 0.5)
    # two-plane views: as before
    fused2, _ = r3d.pipeline.multi_view_fuse_tensors({v: local[v][:2].contiguous() for v in range(3)}, 3, register=register, transform=transform)
    assert fused2.shape == (2, 18, 3) and torch.equal(fused2, fused[:2])
    # plane counts that differ between the views, or that are neither 2 nor 3
    with pytest.raises(ValueError):
        r3d.pipeline.multi_view_fuse_tensors({0: local[0], 1: local[1][:2].contiguous(), 2: local[2]}, 3, register=register, transform=transform)
    with pytest.raises(ValueError):
        r3d.pipeline.multi_view_fuse_tensors({v: torch.zeros((4, 3, 3), dtype=torch.float64) for v in range(3)}, 3,
                                             register=register, transform=transform)
