"""Fixture of the detection data tests: the mini nuScenes of tests/test_reader_cpu.py with the annotation fields of the
reference's converter (tools/data_converter/nuscenes_converter.py:305-332) added and a calibration in which the LiDAR, ego
and global frames really differ (rotations about all three axes).

Every frame carries, next to random boxes: NaN velocities, names outside the ten classes, `valid_flag` false, boxes exactly
on and just outside / inside the BEV bounds, yaws beyond +-pi and exactly +-pi.  Frame EMPTY_FRAME has no valid box at all.
Two scenes: frames 0-5 and 6-(n-1)."""
import pickle

import numpy as np

from test_reader_cpu import _mini_nuscenes

CLASS_NAMES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
               "traffic_cone")
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
SIZES = dict(car=(1.95, 4.6, 1.7), truck=(2.5, 6.9, 2.8), construction_vehicle=(2.8, 6.4, 3.2), bus=(2.9, 11.0, 3.5),
             trailer=(2.9, 12.3, 3.9), barrier=(2.5, 0.5, 1.0), motorcycle=(0.8, 2.1, 1.5), bicycle=(0.6, 1.7, 1.3),
             pedestrian=(0.7, 0.7, 1.8), traffic_cone=(0.4, 0.4, 1.1))
EMPTY_FRAME = 2
N_FRAMES = 16
N_EDGE = 12                                   # the hand-placed boxes at the head of every frame, see `annotations`


def quaternion(roll, pitch, yaw):
    """(w, x, y, z) of Rz(yaw) Ry(pitch) Rx(roll)"""
    cr, sr, cp, sp, cy, sy = (f(a / 2) for a in (roll, pitch, yaw) for f in (np.cos, np.sin))
    return [cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy]


LIDAR2EGO = dict(rotation=quaternion(0.03, -0.02, -1.55), translation=[0.94, 0.1, 1.84])


def ego2global(k):
    return dict(rotation=quaternion(0.015, 0.01 * k - 0.02, 0.4 + 0.05 * k), translation=[600.0 + 2.0 * k, 1600.0 + 0.3 * k, 0.5 + 0.02 * k])


def annotations(k):
    """the annotation fields of frame k"""
    rng = np.random.default_rng(100 + k)
    n = N_EDGE + 6 + k % 3
    names = rng.choice(CLASS_NAMES, n).astype(object)
    xy = rng.uniform(-44.0, 44.0, (n, 2))
    yaw = rng.uniform(-np.pi, np.pi, n)
    vel = rng.normal(0.0, 2.0, (n, 2))
    vel[rng.random(n) < 0.4] *= 0.02                               # slow boxes: the attribute rule has both branches
    valid = np.ones(n, bool)
    lidar_pts = rng.integers(1, 40, n)
    radar_pts = rng.integers(0, 3, n)
    # --- the hand-placed head of the frame
    names[:6] = "car"
    xy[0] = [51.2, 3.0]                                            # exactly on the upper x bound: outside (strict)
    xy[1] = [-51.2, -7.0]                                          # exactly on the lower x bound: outside
    xy[2] = [4.0, 51.2001]                                         # just outside in y
    xy[3] = [51.19, -20.0]; yaw[3] = 3.5                           # just inside; yaw beyond +pi
    xy[4] = [-12.0, -51.19]; yaw[4] = -4.0                         # just inside; yaw beyond -pi
    yaw[5] = np.pi                                                 # wraps to -pi
    names[6], yaw[6] = "pedestrian", -np.pi                        # stays -pi
    names[7] = "animal"                                            # outside the ten classes
    names[8] = "movable_object.debris"
    names[9] = "truck"; valid[9] = False; lidar_pts[9] = 0; radar_pts[9] = 0
    names[10] = "bus"; vel[10] = np.nan                            # NaN velocity on a valid box
    names[11] = "bicycle"; vel[11] = np.nan; valid[11] = False; lidar_pts[11] = 0; radar_pts[11] = 1
    vel[0] = np.nan
    if k == EMPTY_FRAME:
        valid[:] = False
    dims = np.array([SIZES.get(nm, (1.0, 1.0, 1.0)) for nm in names]) * rng.uniform(0.9, 1.1, (n, 1))
    z = rng.uniform(-2.0, 0.5, (n, 1))
    return dict(gt_boxes=np.concatenate([xy, z, dims, yaw[:, None]], 1), gt_names=np.array(names.tolist()),
                gt_velocity=vel, num_lidar_pts=lidar_pts, num_radar_pts=radar_pts, valid_flag=valid)


def det_mini_nuscenes(root, n_frames=N_FRAMES, cams=2):
    """-> path of the info pkl (frames on disk under `root`, infos shuffled: the reader sorts by timestamp)"""
    path = _mini_nuscenes(root, n_frames=n_frames, cams=cams)
    with open(path, "rb") as f:
        data = pickle.load(f)
    for info in data["infos"]:
        k = int(info["token"][3:])
        info.update(annotations(k))
        e2g = ego2global(k)
        info.update(lidar2ego_rotation=list(LIDAR2EGO["rotation"]), lidar2ego_translation=list(LIDAR2EGO["translation"]),
                    ego2global_rotation=e2g["rotation"], ego2global_translation=e2g["translation"])
        info["can_bus"] = np.random.default_rng(300 + k).normal(size=18)
    out = root / "det_infos.pkl"
    with open(out, "wb") as f:
        pickle.dump(data, f)
    return out


def sorted_infos(path):
    with open(path, "rb") as f:
        return sorted(pickle.load(f)["infos"], key=lambda e: e["timestamp"])


def predictions(k, n=40):
    """decoded boxes of frame k as the detector hands them on: LiDAR-frame rows with the z of the bottom face (float32),
    scores, labels; centres out to beyond every class range, speeds on both sides of the 0.2 m/s attribute rule"""
    rng = np.random.default_rng(500 + k)
    labels = rng.integers(0, len(CLASS_NAMES), n)
    dims = np.array([SIZES[CLASS_NAMES[l]] for l in labels]) * rng.uniform(0.8, 1.2, (n, 1))
    vel = rng.normal(0.0, 2.0, (n, 2))
    vel[rng.random(n) < 0.5] *= 0.03
    boxes = np.concatenate([rng.uniform(-55.0, 55.0, (n, 2)), rng.uniform(-3.0, 0.0, (n, 1)), dims,
                            rng.uniform(-4.0, 4.0, (n, 1)), vel], 1).astype(np.float32)
    return dict(boxes=boxes, scores=rng.uniform(0.01, 1.0, n).astype(np.float32), labels=labels.astype(np.int64))


# --- numpy fp64 restatements the tests compare against ---------------------------------------------------------------
def rot(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def yaw_gap(a, b):
    return np.abs((np.asarray(a, np.float64) - np.asarray(b, np.float64) + np.pi) % (2 * np.pi) - np.pi)


def gravity(rows):
    """LiDAR-frame rows with the bottom z (float32) -> the gravity centre, in fp32 like the detector's box class"""
    rows = np.array(rows, np.float32)
    rows[:, 2] = rows[:, 2] + rows[:, 5] * np.float32(0.5)
    return rows


def to_frame(rows, q, t):
    """numpy fp64 restatement of the rigid transform of box rows (heading = the rotated x axis of the box)"""
    h = (-np.asarray(rows, np.float32)[:, 6] - np.pi / 2).astype(np.float64)      # formed in fp32, as the reference forms it
    rows = np.asarray(rows, np.float64)
    R = rot(q)
    head = np.stack([np.cos(h), np.sin(h), np.zeros_like(h)], 1) @ R.T
    vel = np.concatenate([rows[:, 7:9], np.zeros((len(rows), 1))], 1) @ R.T
    return np.concatenate([rows[:, :3] @ R.T + np.asarray(t), rows[:, 3:6],
                           (-np.arctan2(head[:, 1], head[:, 0]) - np.pi / 2)[:, None], vel[:, :2]], 1)
