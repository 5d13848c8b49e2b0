"""A synthetic RGB-D scene for the odometry tests: the height field world z = g(x, y) with a smooth texture, seen by a pinhole
camera that looks along +z.  A frame is rendered per pixel by a ray / surface fixed-point iteration into a depth plane (camera
z, metres) and an intensity plane in [0, 1].  Holes are rectangles: Gaussian3 and the 2x2 mean spread every NaN, so
salt-and-pepper holes leave (almost) nothing on the coarse levels."""
import numpy as np


def height(x, y):
    return 1.5 + 0.10 * np.sin(3.0 * x) * np.cos(2.5 * y) + 0.05 * np.sin(7.0 * x + 1.0) + 0.04 * np.cos(5.0 * y - 0.5)


def texture(x, y):
    return 0.5 + 0.18 * np.sin(9.0 * x + 0.3) * np.cos(7.0 * y) + 0.12 * np.sin(15.0 * y + 4.0 * x) + 0.06 * np.cos(23.0 * x - 11.0 * y)


def camera(w, h):
    """(fx, fy, cx, cy) of a 60 degree wide pinhole"""
    f = 0.5 * w / np.tan(np.radians(30.0))
    return (float(f), float(f), 0.5 * w - 0.5, 0.5 * h - 0.5)


def skewed_camera(w, h):
    """(fx, fy, cx, cy) with fy = 0.85 fx and the principal point 11 % of the width right of and 7 % of the height above the
    centre: a kernel that takes fx for fy, or cx for cy, or assumes a centred principal point gives another answer"""
    f = 0.5 * w / np.tan(np.radians(30.0))
    return (float(f), float(0.85 * f), 0.5 * w - 0.5 + 0.11 * w, 0.5 * h - 0.5 - 0.07 * h)


def pose(rx_deg=0.0, ry_deg=0.0, rz_deg=0.0, t=(0.0, 0.0, 0.0)):
    a, b, c = np.radians([rx_deg, ry_deg, rz_deg])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


def render(w, h, cam_to_world=None, holes=(), step=None, cam=None):
    """-> intensity float32 [h][w], depth float32 [h][w] (0 in the holes).  holes: rectangles (x0, y0, x1, y1) as fractions
    of the image.  step = (x_fraction, dz): columns left of x_fraction see a surface dz nearer (a depth step).
    cam: (fx, fy, cx, cy), camera(w, h) when None."""
    fx, fy, cx, cy = camera(w, h) if cam is None else cam
    C = np.eye(4) if cam_to_world is None else np.asarray(cam_to_world, dtype=np.float64)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    rw = ray @ C[:3, :3].T
    d = np.full((h, w), 1.5)
    for _ in range(40):
        P = rw * d[..., None] + C[:3, 3]
        d = d + (height(P[..., 0], P[..., 1]) - P[..., 2]) / rw[..., 2]
    P = rw * d[..., None] + C[:3, 3]
    inten = texture(P[..., 0], P[..., 1])
    if step is not None:
        near = u < step[0] * w
        d = np.where(near, d - step[1], d)
        inten = np.where(near, 1.0 - inten, inten)
    d = d.astype(np.float32)
    for (x0, y0, x1, y1) in holes:
        d[int(y0 * h):int(y1 * h), int(x0 * w):int(x1 * w)] = 0
    return np.clip(inten, 0.0, 1.0).astype(np.float32), d


HOLES = ((0.10, 0.15, 0.22, 0.30), (0.60, 0.55, 0.78, 0.70))
TRUTH = pose(0.6, -0.7, 0.4, (0.010, -0.008, 0.016))       # about 1 degree and 16 mm from the identity


def pair(w, h, truth=TRUTH, holes=HOLES, cam=None):
    """-> source frame, target frame, camera, truth.  The target camera sits at the world origin, the source camera at
    `truth` (source camera coordinates -> target camera coordinates).  cam: camera(w, h) when None."""
    cam = camera(w, h) if cam is None else tuple(cam)
    return render(w, h, truth, holes, cam=cam), render(w, h, None, holes, cam=cam), cam, np.asarray(truth, dtype=np.float64)
