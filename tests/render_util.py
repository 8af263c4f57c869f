"""Scenes for the tests of tripled_amd.render: points around a short forward-moving, slightly turning trajectory, with the points
planted that decide whether a renderer is right.  Camera 0 is the identity, the focal length a power of two and the principal point a
multiple of one half, so the planted points' projections in camera 0 are exact in float64 and can be stated in advance."""
import collections

import numpy as np

from tripled_amd import render

NEAR, FAR = 0.25, 16.0
SPECIALS = 14        # planted in front of the random points when V holds them and at least as many random ones

Scene = collections.namedtuple("Scene", "xyz rgb poses K near far planted")
Scene.__doc__ = """xyz float32 [V,3], rgb uint8 [V,3], poses float64 [C,3,4], K float64 [3,3];  planted: {} when V is too small for the
special points, else name -> point index (or a tuple), and "tie_pixel" / "half_pixels" -> (v, u) in camera 0."""


def focal(W):
    return float(2 ** int(np.floor(np.log2(max(W, 2)))))


def intrinsics(H, W):
    f = focal(W)
    return np.array([[f, 0.0, 0.5 * (W - 1)], [0.0, f, 0.5 * (H - 1)], [0.0, 0.0, 1.0]])


def trajectory(C):
    """Camera c: 0.3 c forward, drifting 0.02 c to the right, yaw 0.03 c.  Camera 0 is exactly the identity."""
    poses = np.zeros((C, 3, 4))
    for c in range(C):
        a = 0.03 * c
        poses[c, :, :3] = [[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]
        poses[c, :, 3] = [0.02 * c, 0.0, 0.3 * c]
    return poses


def mixed_splat(W):
    """Radius 8 at the depth of the planted near point (0.3125), 6 at the edge straddlers' (0.5), 0 from depth 6 on."""
    return 6.0 / focal(W)


def saturating_splat(W):
    """Radius 8 for every point up to FAR."""
    return 2.0 * FAR * (2 * render.MAX_SPLAT) / focal(W)


def at_pixel(K, u, v, z):
    """The point that camera 0 sees at pixel coordinates (u, v) and depth z: exact for the u, v, z used here."""
    return [z * (u - K[0, 2]) / K[0, 0], z * (v - K[1, 2]) / K[1, 1], z]


def scene(seed, V, C, H, W):
    g = np.random.default_rng(seed)
    K, poses = intrinsics(H, W), trajectory(C)
    f = K[0, 0]
    # random points: a sixth of them inside camera 0's image, a part farther out than the largest square reaches, a part beyond FAR,
    # a part behind the later cameras
    z = g.uniform(0.5, 1.25 * FAR, V)
    x = g.uniform(-1.2, 1.2, V) * (W / f) * z
    y = g.uniform(-1.2, 1.2, V) * (H / f) * z
    xyz = np.stack([x, y, z], 1).astype(np.float32)
    rgb = g.integers(0, 256, (V, 3)).astype(np.uint8)
    planted = {}
    if V >= 2 * SPECIALS:
        tu, tv = float(min(W - 1, W // 2 + 1)), float(H // 2)                 # the tie pixel: an integer position
        ue, uo = float(2 * (W // 4)), float(2 * (W // 4) + 1)                 # u = ue + 0.5 -> ue, u = uo + 0.5 -> uo + 1
        ve, vo = float(2 * (H // 4)), float(2 * (H // 4) + 1)
        special = [
            [np.nan, 0.0, 1.0],                                             # 0  a NaN
            [0.0, 0.0, -1.0],                                               # 1  behind the camera
            [0.0, 0.0, 2.0 * FAR],                                          # 2  beyond far
            at_pixel(K, tu, tv, NEAR),                                      # 3  \ identical: equal z, different index, at z = near
            at_pixel(K, tu, tv, NEAR),                                      # 4  / exactly, nearer than everything else
            at_pixel(K, ue + 0.5, ve + 0.5, 2.0),                           # 5  half to even: down in u and v
            at_pixel(K, uo + 0.5, vo + 0.5, 2.0),                           # 6  half to even: up in u and v
            at_pixel(K, ue + 0.5, vo + 0.5, 2.0),                           # 7  down in u, up in v
            at_pixel(K, uo + 0.5, ve + 0.5, 2.0),                           # 8  up in u, down in v
            at_pixel(K, 0.0, float(H - 1), 0.3125),                         # 9  near enough that mixed_splat reaches MAX_SPLAT
            at_pixel(K, -3.0, float(H // 2), 0.5),                          # 10 \ the centre outside the image, the square of
            at_pixel(K, float(W + 2), float(H // 2), 0.5),                  # 11 | mixed_splat (r = 6) across the left, right, top
            at_pixel(K, float(W // 2), -3.0, 0.5),                          # 12 | and bottom edge
            at_pixel(K, float(W // 2), float(H + 2), 0.5),                  # 13 /
        ]
        assert len(special) == SPECIALS
        xyz[:SPECIALS] = np.array(special, np.float32)
        assert np.array_equal(xyz[1:SPECIALS].astype(np.float64), np.array(special[1:]))      # exact in float32
        planted = dict(nan=0, behind=1, beyond=2, tie=(3, 4), half=(5, 6, 7, 8), near=9, straddle=(10, 11, 12, 13),
                       tie_pixel=(int(tv), int(tu)),
                       half_pixels=((int(ve), int(ue)), (int(vo) + 1, int(uo) + 1), (int(vo) + 1, int(ue)), (int(ve), int(uo) + 1)))
    elif V:
        xyz[0] = [0.0, 0.0, 1.0]                                            # straight ahead of camera 0: something is drawn
    return Scene(xyz, rgb, poses, K, NEAR, FAR, planted)


def modes(W):
    """The four modes of the 3 x (9 x 14) x 700 case: name -> keyword arguments of the renderers."""
    return {"none": dict(splat=0.0), "mixed": dict(splat=mixed_splat(W)), "saturated": dict(splat=saturating_splat(W)),
            "ortho": dict(splat=mixed_splat(W), ortho=True)}


def render_args(s, **over):
    return dict(dict(near=s.near, far=s.far), **over)


def assert_rendered_equal(got, want):
    for name, a, b in zip(render.Rendered._fields, got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), "%s differs at %d places" % (name, int(np.count_nonzero(a != b)))
