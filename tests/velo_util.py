"""Synthetic KITTI calibrations and velodyne scans for the tests of tripled_amd.velodyne (CPU, GPU, against the reference) and for
tools/gen_golden_velo.py / tools/velo_bench.py.  Nothing here is measured data: a calibration is a pinhole camera of the requested
size behind a slightly rotated, slightly shifted sensor, and a scan is drawn so that it exercises every rule of the depth map:
several points per pixel, points on the last column next to points on the first column of the next row (the reference's group
index joins them), points behind the sensor, outside the image, with a negative depth inside it, NaN / inf coordinates, x = -0.0."""
import os

import numpy as np

GOLDEN_SCENES = (("a", 9, 14, 400, 1), ("b", 12, 33, 3000, 2))      # name, H, W, points, seed
CALIB_KEYS = ("S_rect_02", "P_rect_02", "P_rect_03", "R_rect_00", "R", "T")


def _small_rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz.dot(Ry.dot(Rx))


def synthetic_calibration(H, W, seed=0):
    """The numbers of calib_cam_to_cam.txt / calib_velo_to_cam.txt that generate_depth_map reads, as float64 arrays (flat, as a
    calibration file lists them).  Every number is rounded to 7 significant digits, like a KITTI file's '%e' fields."""
    g = np.random.default_rng(seed)
    fx, fy, cx, cy = 0.58 * W, 1.92 * H, 0.5 * W, 0.5 * H
    P2 = np.array([[fx, 0, cx, 0.06 * fx], [0, fy, cy, 0.002 * fy], [0, 0, 1, 0.003]])
    P3 = np.array([[fx, 0, cx, -0.47 * fx], [0, fy, cy, 0.002 * fy], [0, 0, 1, 0.003]])
    axes = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])          # velodyne (fwd, left, up) -> camera (right, down, fwd)
    R = _small_rotation(*g.normal(0, 0.01, 3)).dot(axes)
    T = np.array([0.004, -0.07, -0.27]) + g.normal(0, 0.005, 3)
    out = {"S_rect_02": np.array([float(W), float(H)]), "P_rect_02": P2.reshape(-1), "P_rect_03": P3.reshape(-1),
           "R_rect_00": _small_rotation(*g.normal(0, 0.005, 3)).reshape(-1), "R": R.reshape(-1), "T": T}
    return {k: np.array([float("%.6e" % v) for v in out[k]]) for k in CALIB_KEYS}


def projection(calib, cam=2):
    from tripled_amd import velodyne
    return velodyne.projection_matrix(calib["P_rect_0%d" % cam], calib["R_rect_00"], calib["R"], calib["T"])


def size_of(calib):
    return int(calib["S_rect_02"][1]), int(calib["S_rect_02"][0])


def synthetic_scan(calib, n, seed=0, specials=True):
    """float32 [n,4]: points aimed at pixels of an area a little larger than the image, at depths of 2 ... 60 m (a quarter of them on
    a 0.25 m lattice, so that depths tie), with the special points sprinkled in when there is room for them (n >= 64)."""
    g = np.random.default_rng(seed)
    H, W = size_of(calib)
    fx, fy, cx, cy = 0.58 * W, 1.92 * H, 0.5 * W, 0.5 * H
    u = g.uniform(-0.08 * W, 1.08 * W, n)
    v = g.uniform(-0.08 * H, 1.08 * H, n)
    # a third of the points sit on the two columns where the group index joins a row's end to the next row's start
    edge = g.random(n) < 0.33
    u = np.where(edge, np.where(g.random(n) < 0.5, W + g.uniform(-0.45, 0.45, n), 1 + g.uniform(-0.45, 0.45, n)), u)
    Z = g.uniform(2.0, 60.0, n)
    Z = np.where(g.random(n) < 0.25, np.round(Z * 4) / 4, Z)
    pts = np.stack([Z + 0.27, -(u - cx) * Z / fx, -(v - cy) * Z / fy - 0.07, g.random(n)], 1).astype(np.float32)
    if specials and n >= 64:
        n_near = max(27, n // 100)
        at = g.permutation(n)[:13 + n_near]
        pts[at[0:8], 0] = -np.abs(pts[at[0:8], 0])                                  # behind
        pts[at[8], 0] = np.nan
        pts[at[9], 1] = np.nan
        pts[at[10], 2] = np.inf
        pts[at[11], 0] = np.inf
        pts[at[12]] = (-0.0, 0.0, 0.0, 0.5)                                        # kept by x >= 0
        # in front of the sensor but behind the camera: a negative depth, and pixels inside the image for some of them (half of
        # them spread over the width of camera 3's baseline shift)
        near = at[13:]
        wide = np.where(np.arange(len(near)) % 2 == 0, 0.08, 0.6)
        pts[near, 0] = g.uniform(0.0, 0.2, len(near)).astype(np.float32)
        pts[near, 1] = (wide * g.uniform(-1.0, 1.0, len(near))).astype(np.float32)
        pts[near, 2] = g.uniform(-0.12, -0.02, len(near)).astype(np.float32)
    return pts


def write_calib(calib_dir, calib):
    """The two calibration files of a KITTI date directory; 17 significant digits, so that reading them returns the arrays."""
    os.makedirs(calib_dir, exist_ok=True)

    def line(key, values):
        return "%s: %s\n" % (key, " ".join("%.16e" % v for v in values))

    with open(os.path.join(calib_dir, "calib_cam_to_cam.txt"), "w") as f:
        f.write("calib_time: 09-Jan-2012 13:57:47\ncorner_dist: 9.950000e-02\n")
        for key in ("S_rect_02", "R_rect_00", "P_rect_02", "P_rect_03"):
            f.write(line(key, calib[key]))
    with open(os.path.join(calib_dir, "calib_velo_to_cam.txt"), "w") as f:
        f.write("calib_time: 15-Mar-2012 11:37:16\n")
        f.write(line("R", calib["R"]) + line("T", calib["T"]))


def write_scan(root, folder, frame_index, points):
    path = os.path.join(root, folder, "velodyne_points", "data", "{:010d}.bin".format(int(frame_index)))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.ascontiguousarray(points, dtype=np.float32).tofile(path)
    return path


def false_collisions(points, P, H, W):
    """How many duplicate groups of the scan hold points of two different pixels (the reference's index joins pixel (v, W-1) and
    pixel (v+1, 0)), and how many duplicate groups there are: what a fixture must have to exercise the rule."""
    pts = np.asarray(points, np.float32)
    keep = pts[:, 0] >= 0
    x, y, z = (pts[keep, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        r = [((P[k, 0] * x + P[k, 1] * y) + P[k, 2] * z) + P[k, 3] for k in range(3)]
        u, v = np.rint(r[0] / r[2]) - 1, np.rint(r[1] / r[2]) - 1
        ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    u, v = u[ok].astype(np.int64), v[ok].astype(np.int64)
    g = v * (W - 1) + u
    members = np.bincount(g, minlength=H * (W - 1) + 1)
    on_first_column = np.bincount(g, weights=(u == 0), minlength=len(members))
    mixed = (members > 1) & (on_first_column > 0) & (on_first_column < members) & (np.arange(len(members)) > 0)
    return int(np.count_nonzero(mixed)), int(np.count_nonzero(members > 1))


# ---------------------------------------------------------------------------------------------------------------------------
# hand-made cases: the expected maps are written down by hand from the rules, not computed

PERMUTE = np.array([[0.0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]])              # r = (y, z, x): u = rint(y / x) - 1, v = rint(z / x) - 1, d = x
PERMUTE_MINUS_ONE = np.array([[0.0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, -1]])   # r_2 = x - 1: negative for 0 <= x < 1
PERMUTE_PLUS_ONE = np.array([[0.0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 1]])     # r_2 = x + 1
_NAN, _INF = float("nan"), float("inf")


def _pts(rows):
    return np.array([list(r) + [0.5] for r in rows], dtype=np.float32).reshape(-1, 4)


def hand_cases():
    """name -> (points, P, H, W, vel_depth, {(v, u): depth} of the non-zero pixels, stats)."""
    on_last_column, on_next_row = (2, 8, 2), (5, 5, 10)      # H x W = 3 x 4: pixel (0, 3) at d = 2 and pixel (1, 0) at d = 5 share group 2
    return {
        # 5 / 2 = 2.5 rounds to 2 (column 1), 7 / 2 = 3.5 rounds to 4 (column 3)
        "half_to_even": (_pts([(2, 5, 2), (2, 7, 2)]), PERMUTE, 2, 6, False, {(0, 1): 2.0, (0, 3): 2.0}, [2, 0, 0, 2, 2, 0]),
        # the group's first point is the near one: its pixel gets min(2, 5) = 2, the other pixel keeps its own 5
        "false_collision": (_pts([on_last_column, on_next_row]), PERMUTE, 3, 4, False, {(0, 3): 2.0, (1, 0): 5.0}, [2, 0, 0, 2, 2, 0]),
        # the far one first: ITS pixel is overwritten with the other pixel's nearer depth
        "false_collision_reversed": (_pts([on_next_row, on_last_column]), PERMUTE, 3, 4, False, {(0, 3): 2.0, (1, 0): 2.0},
                                     [2, 0, 0, 2, 2, 0]),
        # group 2 = {(1,0) d 5, (0,3) d 3, (0,3) d 6}: pixel (1,0) gets the minimum 3; pixel (0,3) keeps its LAST point, 6, not its nearest
        "last_write_wins": (_pts([on_next_row, (3, 12, 3), (6, 24, 6)]), PERMUTE, 3, 4, False, {(0, 3): 6.0, (1, 0): 3.0}, [3, 0, 0, 3, 2, 0]),
        # pixel (0,0) is group -1: three points, the last is 3, the group minimum 2 wins
        "pixel_00": (_pts([(4, 4, 4), (2, 2, 2), (3, 3, 3)]), PERMUTE, 2, 3, False, {(0, 0): 2.0}, [3, 0, 0, 3, 1, 0]),
        # x = 0.5: r = (-1, -0.5, -0.5): pixel (0, 1) at depth -0.5, clamped to 0 and counted
        "negative_depth": (_pts([(0.5, -1, -0.5)]), PERMUTE_MINUS_ONE, 2, 3, False, {}, [1, 0, 0, 1, 1, 1]),
        # the same point with vel_depth: d = x = 0.5
        "negative_depth_vel": (_pts([(0.5, -1, -0.5)]), PERMUTE_MINUS_ONE, 2, 3, True, {(0, 1): 0.5}, [1, 0, 0, 1, 1, 0]),
        # a negative depth takes part in the group minimum: pixel (0, 1) is hit at -0.5, then at 2; the last write is 2, the group's
        # minimum -0.5 replaces it and is clamped to 0
        "negative_in_group": (_pts([(0.5, -1, -0.5), (3, 4, 2)]), PERMUTE_MINUS_ONE, 2, 3, False, {}, [2, 0, 0, 2, 1, 1]),
        # r_2 = 0 (inf and NaN quotients), NaN / inf coordinates: all outside
        "degenerate": (_pts([(0, 1, 1), (0, 0, 0), (1, _NAN, 1), (1, 1, _INF), (_NAN, 1, 1), (_INF, 1, 1)]), PERMUTE, 2, 3, False, {},
                       [6, 0, 6, 0, 0, 0]),
        # x = -0.0 passes x >= 0: r_2 = 1, pixel (0, 1)
        "minus_zero": (_pts([(-0.0, 2, 1), (-1.0, 2, 1)]), PERMUTE_PLUS_ONE, 2, 3, False, {(0, 1): 1.0}, [2, 1, 0, 1, 1, 0]),
        "no_points": (_pts([]), PERMUTE, 2, 3, False, {}, [0, 0, 0, 0, 0, 0]),
        "none_valid": (_pts([(-1, 1, 1), (-2, 2, 2), (1, 50, 1)]), PERMUTE, 2, 3, False, {}, [3, 2, 1, 0, 0, 0]),
    }


def hand_expected(case):
    _, _, H, W, _, pixels, stats = case
    depth = np.zeros((H, W), np.float64)
    for (v, u), d in pixels.items():
        depth[v, u] = d
    return depth, np.array(stats, np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# a tiny raw KITTI tree

TREE_DATES = (("2011_09_26", 30, 52, 900, 11), ("2011_09_28", 27, 47, 700, 12))      # date, H, W, points per scan, seed


def make_kitti_tree(root, frames_per_drive=1):
    """Two dates with calibrations of different sizes, one drive each: colour frames of the calibration's size (image_02 and
    image_03, PNG), velodyne scans and the calibration files.  Returns (split lines alternating between the dates and the sides,
    {line: (points, calibration)})."""
    from PIL import Image
    from tests.infer_util import smooth_image
    lines, truth = [], {}
    for date, H, W, n, seed in TREE_DATES:
        calib = synthetic_calibration(H, W, seed)
        write_calib(os.path.join(root, date), calib)
        folder = "%s/%s_drive_0001_sync" % (date, date)
        for i in range(frames_per_drive):
            points = synthetic_scan(calib, n, seed * 10 + i)
            write_scan(root, folder, i, points)
            side = "l" if (i + seed) % 2 else "r"
            for cam in (2, 3):
                d = os.path.join(root, folder, "image_0%d" % cam, "data")
                os.makedirs(d, exist_ok=True)
                Image.fromarray(smooth_image(seed * 100 + 10 * i + cam, H, W)).save(os.path.join(d, "%010d.png" % i))
            line = "%s %d %s" % (folder, i, side)
            lines.append(line)
            truth[line] = (points, calib)
    return lines, truth
