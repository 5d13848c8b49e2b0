"""CPU tests of tests/poisson_ref.py, the numpy restatement of the Poisson reconstruction contract: its two
forms agree bit for bit, and on a sphere the result is the sphere: zero level set within half a cell, a converging solver, a closed
outward-facing mesh of genus 0."""
import numpy as np
import pytest

from tests import poisson_ref as ref
from tests.tsdf_mesh_ref import edge_census, signed_volume

RADIUS = 0.7


@pytest.fixture(scope="module")
def table(r3d):
    return r3d.tsdf.mc_table()          # host only: no device


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_the_two_forms_agree_bit_for_bit(table, depth):
    pts, nrm, col = ref.sphere_cloud(150, RADIUS, noise=0.01, seed=depth)
    pts[-1] = pts[0]                    # the same point twice
    p = ref.params(depth=depth, cycles=2, coarse_sweeps=6)
    A = ref.fields(pts, nrm, col, p)
    B = ref.fields(pts, nrm, col, p, literal=True)
    for name in ("W0", "C0", "dens", "V", "D", "b", "chi"):
        assert _same(A[name], B[name]), name
    assert np.abs(A["chi"]).max() > 0
    ma = ref.extract(A["chi"], A["W0"], A["C0"], A["org"], A["h"], table)
    mb = ref.extract_literal(B["chi"], B["W0"], B["C0"], B["org"], B["h"], table)
    assert len(ma[3]) > 0
    for x, y in zip(ma, mb):
        assert _same(x, y)
    nc = ref.extract(A["chi"], A["W0"], None, A["org"], A["h"], table)
    assert nc[2] is None and _same(nc[0], ma[0]) and _same(nc[3], ma[3])


@pytest.fixture(scope="module")
def sphere(table):
    """a 4 000-point sphere of radius 0.7 at depth 5, with chi after every cycle.  The points are a Fibonacci lattice: 0.039 apart
    at h = 0.048, so every surface cell holds a sample and the half-cell bound tests the discretisation.  (4 000 RANDOM points
    leave a fifth of the surface cells empty; the restatement then puts 13 to 22 of its 4 050 vertices up to 1.6 h off, where the
    thin outside layer of chi dips below zero next to the grid's face.)"""
    pts, nrm, col = ref.sphere_cloud(4000, RADIUS, lattice=True)
    p = ref.params(depth=5)
    history = []
    S = ref.fields(pts, nrm, col, p, history=history)
    vert, dens, vcol, tri = ref.extract(S["chi"], S["W0"], S["C0"], S["org"], S["h"], table)
    return dict(S=S, p=p, history=history, vert=vert, dens=dens, col=vcol, tri=tri)


def test_zero_level_set_is_within_half_a_cell_of_the_sphere(sphere):
    h = sphere["S"]["h"]
    err = np.abs(np.linalg.norm(sphere["vert"], axis=1) - RADIUS) / h
    print(f"vertex radius error: max {err.max():.3f} h, mean {err.mean():.3f} h over {len(err)} vertices")
    assert len(err) > 0 and err.max() <= 0.5


def test_chi_is_negative_inside(sphere):
    S = sphere["S"]
    G = S["G"]
    centre = np.round((0.0 - S["org"]) / S["h"]).astype(int)
    assert S["chi"][centre[2], centre[1], centre[0]] < 0
    assert S["chi"][1, 1, 1] > 0 and S["chi"][G - 2, G - 2, G - 2] > 0


def test_residual_falls_every_cycle_and_ends_below_one_percent(sphere):
    S, p = sphere["S"], sphere["p"]
    ratios = [ref.residual_ratio(x, S["b"], S["D"], p["alpha"]) for x in sphere["history"]]
    print("interior residual ratio per cycle:", " ".join(f"{r:.3e}" for r in ratios))
    assert len(ratios) == 10
    for c in range(1, 10):
        assert ratios[c] < ratios[c - 1], c
    assert ratios[-1] < 1e-2


def test_mesh_is_closed_of_genus_zero_and_faces_outward(sphere):
    vert, tri = sphere["vert"], sphere["tri"]
    repeated, boundary, undirected = edge_census(tri)
    assert repeated == 0 and boundary == 0
    assert len(vert) - undirected + len(tri) == 2
    assert len(np.unique(tri)) == len(vert) and tri.min() == 0 and tri.max() == len(vert) - 1
    assert signed_volume(vert, tri) > 0
    assert sphere["dens"].shape == (len(vert),) and (sphere["dens"] > 0).all()
    assert sphere["col"].shape == vert.shape and np.isfinite(sphere["col"]).all()
