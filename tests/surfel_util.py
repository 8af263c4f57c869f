"""Scenes for the tests of the surfel renderer and of the orientation of normals: tests/render_util.py's scene with a normal per point
and five more planted points.  Camera 0 is the identity, so a planted normal is its own camera-space normal there, exactly."""
import collections

import numpy as np

from tests import render_util as U
from tripled_amd import render

NEAR, FAR = U.NEAR, U.FAR
SPECIALS = U.SPECIALS + 5
RADIUS = 0.375       # exact in binary.  Perspective, focal 8, near 0.25: g = radius / near = 1.5 for a disc that reaches nearer than near,
                     # the bound 12 (1 + |q0| / z) pixels: capped off axis.  Orthographic, focal 8: r = 3 for every disc

Scene = collections.namedtuple("Scene", "xyz rgb normals poses K near far planted")
Scene.__doc__ = """render_util.Scene with normals float32 [V,3] (random unit vectors, half of them facing away from camera 0; zero for the
planted point without one).  planted: render_util's names, plus facing, edge_on, back, bare, capped -> point index, and "facing_pixel"
-> (v, u) in camera 0."""


def scene(seed, V, C, H, W):
    """H odd: K12 is then an integer, and the ray through a pixel of the middle row has d1 = 0 exactly."""
    s = U.scene(seed, V, C, H, W)
    g = np.random.default_rng(seed + 1000)
    n = g.normal(size=(V, 3))
    normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32) if V else np.zeros((0, 3), np.float32)
    xyz, planted = s.xyz.copy(), dict(s.planted)
    if s.planted and V >= 2 * SPECIALS:
        assert H % 2 == 1
        at = U.SPECIALS
        fu, fv = float(W // 2), float(H // 2)
        special = [
            (U.at_pixel(s.K, fu, fv, 1.0), [0.0, 0.0, -1.0]),                # 14 a disc exactly facing camera 0 at an integer pixel
            (U.at_pixel(s.K, fu - 2.0, fv, 1.5), [0.0, 1.0, 0.0]),           # 15 edge-on: den = 0 at its centre pixel (d1 = 0, m = (0, 1, 0))
            (U.at_pixel(s.K, fu + 1.0, fv - 1.0, 0.75), [0.0, 0.0, 1.0]),    # 16 back-facing, nearer than the facing one
            (U.at_pixel(s.K, fu - 1.0, fv + 1.0, 0.875), [0.0, 0.0, 0.0]),   # 17 without a normal: a billboard
            (U.at_pixel(s.K, 1.0, 1.0, 0.3125), [0.0, 0.0, -1.0]),           # 18 z - RADIUS < near and off axis: the bound passes the cap
        ]
        for j, (p, m) in enumerate(special):
            xyz[at + j], normals[at + j] = np.array(p, np.float32), np.array(m, np.float32)
            assert np.array_equal(xyz[at + j].astype(np.float64), np.array(p))      # exact in float32
        planted.update(facing=at, edge_on=at + 1, back=at + 2, bare=at + 3, capped=at + 4, facing_pixel=(int(fv), int(fu)))
    else:
        planted = {}
    return Scene(xyz, s.rgb, normals, s.poses, s.K, s.near, s.far, planted)


def modes():
    """The eight modes of the 3 x (9 x 14) x 700 case: name -> keyword arguments of the surfel renderers."""
    return {"%s-%s-%s" % ("ortho" if o else "persp", "cull" if c else "all", "lit" if a < 1 else "flat"): dict(ortho=o, cull=c, ambient=a)
            for o in (False, True) for c in (False, True) for a in (1.0, 0.25)}


def args(s, radius=RADIUS, **over):
    """(positional, keyword) arguments of render_surfels_numpy / _bruteforce / _hip after (H, W)."""
    return dict(dict(radius=radius, near=s.near, far=s.far), **over)


def wide_scene(seed, V, C, H, W):
    """Surfels all over and around the image, up to 1.6 times its half-extent off axis, none nearer than 2: with radius 0.4 and focal
    8 the bound stays below 8 (1 + 1.6 W / 16) 0.4 / 1.6 + 1 < MAX_SURFEL for W <= 14: no cap.  Random normals, grazing ones included."""
    g = np.random.default_rng(seed)
    K, poses = U.intrinsics(H, W), U.trajectory(C)
    f = K[0, 0]
    z = g.uniform(2.0, 10.0, V)
    x = g.uniform(-1.6, 1.6, V) * (0.5 * W / f) * z
    y = g.uniform(-1.6, 1.6, V) * (0.5 * H / f) * z
    n = g.normal(size=(V, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[: V // 8, 2] *= 0.02                                                  # nearly edge-on for a camera looking along z
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    for j, (cu, cv) in enumerate(((-2.0, -2.0), (W + 1.0, -2.0), (-2.0, H + 1.0), (W + 1.0, H + 1.0))):      # beyond the four corners
        x[j], y[j], z[j] = 2.0 * (cu - K[0, 2]) / f, 2.0 * (cv - K[1, 2]) / f, 2.0
        n[j] = [0.0, 0.0, -1.0]
    return Scene(np.stack([x, y, z], 1).astype(np.float32), g.integers(0, 256, (V, 3)).astype(np.uint8), n.astype(np.float32), poses, K,
                 NEAR, FAR, {})


def plane_scene():
    """Test C's input: camera at the origin, 9 x 14, focal 8; a plane through (0, 0, 3) with normal ~ (0.3, -0.2, -1) sampled on a 49 x 49
    lattice of spacing 0.5 (in-plane axes: normal x (0, 1, 0), and normal x that), and one point behind it without a normal.
    -> (Scene, unit normal float64, index of the far point)."""
    H, W = 9, 14
    K = np.array([[8.0, 0.0, 0.5 * (W - 1)], [0.0, 8.0, 0.5 * (H - 1)], [0.0, 0.0, 1.0]])
    nrm = np.array([0.3, -0.2, -1.0])
    nrm /= np.linalg.norm(nrm)
    a = np.cross(nrm, [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    ij = (np.arange(49) - 24) * 0.5
    lattice = (np.array([0.0, 0.0, 3.0]) + ij[:, None, None] * a + ij[None, :, None] * b).reshape(-1, 3)
    xyz = np.concatenate([lattice, [[0.05, 0.03, 6.0]]]).astype(np.float32)
    normals = np.concatenate([np.tile(nrm, (len(lattice), 1)), [[0.0, 0.0, 0.0]]]).astype(np.float32)
    rgb = np.random.default_rng(3).integers(0, 256, xyz.shape).astype(np.uint8)
    return Scene(xyz, rgb, normals, np.eye(4)[None, :3].copy(), K, NEAR, FAR, {}), nrm, len(lattice)


def assert_surfels_equal(got, want):
    for name, a, b in zip(render.SurfelRendered._fields, got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), "%s differs at %d places" % (name, int(np.count_nonzero(a != b)))
