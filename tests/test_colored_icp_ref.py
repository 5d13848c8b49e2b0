"""CPU checks of the coloured-ICP restatement (tests/colored_icp_ref.py) the GPU tests compare the HIP kernels with: the
gradient set-up on fields whose gradient is known, the zero-gradient rule, what the photometric term buys on a flat textured
patch, and lambda = 1 falling back to the oracle's point-to-plane loop."""
import numpy as np

from oracle import cloud_oracle as co
from tests import colored_icp_ref as cr


def test_gradient_of_a_linear_field_on_an_exact_plane():
    rng = np.random.default_rng(1)
    n = np.array([0.3, -0.5, 0.8])
    n /= np.linalg.norm(n)
    u = np.cross(n, [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    ab = rng.uniform(-0.2, 0.2, (1500, 2))
    pts = 0.7 * n + ab[:, :1] * u + ab[:, 1:] * v
    g = np.array([1.3, -0.7, 0.4])                       # field gradient in space; only its tangential part is observable
    inten = 0.5 + pts @ g
    _, grad, cnt = cr.color_gradients(pts, np.broadcast_to(n, pts.shape), cr.colors_of(inten), 0.05, 30)
    solved = cnt >= 4
    assert solved.sum() > 1400
    g_tan = g - (g @ n) * n
    # bound: the cofactor inverse loses cond(A^T A)^2 when one rank-one term dominates; here the last row contributes 29^2 = 841
    # along the normal, the 29 tangent rows about 29 * (0.02 m)^2 = 0.012, so cond^2 * 2^-53 = (7e4)^2 * 1.1e-16 = 5e-7 on |g| = 1
    assert np.abs(grad[solved] - g_tan).max() < 1e-6
    assert np.abs(grad[solved] @ n).max() < 1e-6
    assert (grad[~solved] == 0).all()


def test_sparse_cloud_has_zero_and_solved_gradients():
    rng = np.random.default_rng(2)
    pts = rng.uniform(0, 2, (300, 3))
    nrm = rng.standard_normal((300, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    _, grad, cnt = cr.color_gradients(pts, nrm, rng.uniform(0, 1, (300, 3)), 0.2, 30)
    few = cnt < 4
    assert 200 < few.sum() < 300                         # both kinds present (this seed: 273 of 300 without a gradient)
    assert (grad[few] == 0).all()
    assert (np.abs(grad[~few]).max(1) > 0).all() and np.isfinite(grad).all()


def test_colour_stops_the_slide_on_a_flat_textured_patch():
    s, sc, t, tn, tc, T = cr.scene(relief=0.0)
    plane = co.registration(s, t, 0.02, mode="p2plane", max_iteration=50, target_normals=tn)
    col = cr.registration_colored(s, sc, t, tn, tc, 0.02, max_iteration=50)
    e_plane, e_col = cr.pose_error(plane["T"], T)[0], cr.pose_error(col["T"], T)[0]
    print(f"translation error: point-to-plane {e_plane * 1e3:.3f} mm after {plane['iterations']} iterations, "
          f"coloured {e_col * 1e3:.4f} mm after {col['iterations']}")
    assert e_col < 0.1 * e_plane
    assert e_col < 1e-4 and col["iterations"] <= 5


def test_lambda_one_is_point_to_plane_iteration_for_iteration():
    s, sc, t, tn, tc, _ = cr.scene(relief=1e-3)
    for max_it in (1, 2, 4, 30):
        want = co.registration(s, t, 0.02, mode="p2plane", max_iteration=max_it, target_normals=tn)
        got = cr.registration_colored(s, sc, t, tn, tc, 0.02, lambda_geometric=1.0, max_iteration=max_it)
        assert got["iterations"] == want["iterations"] and got["correspondences"] == want["correspondences"]
        assert np.abs(got["T"] - want["T"]).max() < 1e-12
