"""The pose family of the camera-move tests (tests/test_set_camera_cpu.py keeps its ledger, tests/test_gpu_set_camera.py walks it): for a
scene's camera record and primitives, a seeded list of (label, camera record) that a camera drag could pass through -- and the places
where the face certificate of the camera rays' work list (csrc/pt_camera_faces.h) changes its answer.  Pure numpy, no renderer.

    own              the scene's own pose
    side_0.3, side_1 sidesteps along the camera's right
    dolly_0.52, dolly_0.505
                     the eye moved to 0.52 / 0.505 object units from the centre plane of the scene's first thin wall, along that wall's thin
                     axis, on the room's side: either side of the certificate's condition (ii), s o_K >= 1/2 + 1e-2 + inset
    yaw_5, yaw_30, yaw_90
                     the view turned about `up`
    graze            an eye three object units off that wall's centre plane, looking along the wall with a slope of 5e-4 towards it: the
                     certificate's slope bound |q_K| >= 1e-3 |q|
    outside          an eye far outside the room, looking at its centre from the side
    turned_back      the scene's eye looking the other way: primitives behind the eye, whose rectangles are the whole frame
    away             an eye 30 units back, the view turned by 80 degrees: every primitive in front of it and off the frame -- it sees nothing,
                     the scene rectangle is empty
    rand_0, rand_1   seeded: an eye inside the primitives' bounding box, a random view
"""
import zlib

import numpy as np

SCENES = ("cornell.txt", "cornell_glass.txt", "room_tilted.txt")
SIZES = ((97, 61), (130, 70))


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _rotate(v, axis, deg):
    """Rodrigues: v turned by deg about the unit axis"""
    a, c, s = _unit(axis), np.cos(np.radians(deg)), np.sin(np.radians(deg))
    v = np.asarray(v, np.float64)
    return v * c + np.cross(a, v) * s + a * np.dot(a, v) * (1.0 - c)


def _thin_wall(geoms):
    """(index, thin axis, 3 x 3 linear part and translation of its transform) of the scene's side wall: of the thin cubes the one that
    stands farthest from the plane x = 0, the first of them"""
    best = None
    for i in range(len(geoms)):
        sc = np.abs(np.asarray(geoms["scale"][i], np.float64))
        if int(geoms["type"][i]) == 1 and sc.min() <= 0.06 and np.sort(sc)[1] >= 1.0:
            x = abs(float(geoms["translation"][i][0]))
            if best is None or x > best[0]:
                best = (x, i, int(sc.argmin()))
    if best is None:
        raise ValueError("the scene has no thin wall")
    _, i, K = best
    m = np.asarray(geoms["transform"][i], np.float64).reshape(4, 4).T                  # (column-major in the record)
    return i, K, m[:3, :3], m[:3, 3]


def poses(name, camera, geoms):
    """[(label, camera record)] for the scene `name` (the seed), its camera record at the size wanted, and its primitives"""
    cam0 = np.array(camera, copy=True).reshape(1)
    eye = np.asarray(cam0["position"][0], np.float64)
    view = np.asarray(cam0["view"][0], np.float64)
    up = np.asarray(cam0["up"][0], np.float64)
    right = _unit(np.cross(view, up))
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    centre = np.asarray(geoms["translation"], np.float64).mean(axis=0)
    lo, hi = np.asarray(geoms["translation"], np.float64).min(axis=0), np.asarray(geoms["translation"], np.float64).max(axis=0)
    _, K, M, t = _thin_wall(geoms)
    side = 1.0 if np.dot(M[:, K], centre - t) > 0 else -1.0          # the room's side of the wall

    out = []

    def add(label, e=None, v=None, u=None):
        c = cam0.copy()
        if e is not None:
            c["position"][0] = np.asarray(e, np.float32)
        if v is not None:
            c["view"][0] = np.asarray(v, np.float32)
        if u is not None:
            c["up"][0] = np.asarray(u, np.float32)
        out.append((label, c))

    add("own")
    add("side_0.3", eye + 0.3 * right)
    add("side_1", eye + 1.0 * right)
    for d in (0.52, 0.505):
        o = np.array([0.3, 0.2, 0.1])
        o[K] = side * d
        add("dolly_%g" % d, M @ o + t)
    for deg in (5, 30, 90):
        add("yaw_%d" % deg, v=_rotate(view, up, deg))
    along = (K + 2) % 3
    o = np.array([0.05, -0.1, 0.02])
    o[K] = side * 3.0
    o[along] = -0.3
    add("graze", M @ o + t, _unit(_unit(M[:, along]) - side * 5e-4 * _unit(M[:, K])), up if abs(np.dot(_unit(M[:, along]), _unit(up))) < 0.9 else right)
    far = centre + 30.0 * right + 0.5 * _unit(up)
    add("outside", far, _unit(centre - far))
    add("turned_back", v=-view)
    add("away", eye - 30.0 * _unit(view), _rotate(view, up, 80))
    for k in range(2):
        e = lo + (hi - lo) * rng.uniform(0.15, 0.85, 3)
        v = _unit(rng.normal(size=3))
        u = up if abs(np.dot(v, _unit(up))) < 0.9 else right
        add("rand_%d" % k, e, v, u)
    return out


def family(pt, scenes_dir):
    """every (scene name, W, H, label, camera record, geoms) of the family, the scenes loaded through the package `pt`"""
    import os
    for name in SCENES:
        for W, H in SIZES:
            sc = pt.Scene(os.path.join(scenes_dir, name))
            sc.set_resolution(W, H)
            geoms = sc.geoms.view(pt.GEOM_DTYPE)
            for label, cam in poses(name, sc.camera.view(pt.CAMERA_DTYPE), geoms):
                yield name, W, H, label, cam, geoms


def dump(path):
    """The family as tests/sanitize_camera_list.hip reads it: int32 records, then per record the camera record, int32 ngeoms, the geoms"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    pt = ge.load_package()
    records = list(family(pt, os.path.join(root, "scenes")))
    with open(path, "wb") as f:
        f.write(np.int32(len(records)).tobytes())
        for _, _, _, _, cam, geoms in records:
            f.write(np.ascontiguousarray(cam).tobytes())
            f.write(np.int32(len(geoms)).tobytes())
            f.write(np.ascontiguousarray(geoms).tobytes())
    return len(records)


if __name__ == "__main__":
    import sys
    print("%d poses written to %s" % (dump(sys.argv[1]), sys.argv[1]))
