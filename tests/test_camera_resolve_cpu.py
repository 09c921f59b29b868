"""The face certificate of the camera rays' work list (pt_init's camera_face_certificate / build_camera_list, host code) against the
oracle's own box test: a wave that pt_init resolves to (cube g, face) promises that EVERY camera ray of every one of its pixels hits g,
from outside, through that face -- the kernel then skips the slab test for it.  So for every resolved pixel (a fixed seeded sample of at
most 20 000 per case, all of them where there are fewer) the oracle's camera ray of iterations 1..8, and float32 rays through the four
corners and the four edge midpoints of the unit pixel square, go through the oracle's `intersect`: hit, outside, the certified face's
normal.  No violation, no ray skipped.  Cornell, the glass box and the room of rotated walls, at the benchmark's shapes and at small
awkward ones; in shards of 1, 2, 3 and 8 members, whose resolved pixels together are the unsharded list's.

The footprint margin of the certificate is 2 px (the spans' own), for which the float64 prototype resolved 0.864 / 0.889 / 0.342 of
the listed pixels of Cornell 1280x720 / the glass box 1920x1080 / Cornell 97x61; the floors asserted here are 0.80 / 0.80 / 0.25."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 0xFFFFFFFF
SAMPLE = 20000

# (scene, W, H, least resolved share of the listed pixels or None)
CASES = [
    ("cornell.txt", 1280, 720, 0.80), ("cornell.txt", 97, 61, 0.25), ("cornell.txt", 40, 30, None),
    ("cornell_glass.txt", 1920, 1080, 0.80), ("cornell_glass.txt", 63, 200, None), ("room_tilted.txt", 97, 61, None),
]


def _resolved(pt, cam, geoms, rank, count):
    """The pixels of one shard's resolved waves -- (pixel index, primitive, face) per pixel, sorted by pixel -- and the number of listed
    pixels."""
    got = pt.camera_resolved(cam, geoms, rank, count)
    assert got is not None
    pix, wave, sig, face = got
    assert face.shape == (len(pix) // 64,) and np.all((face >= -1) & (face <= 5))
    W = int(cam["resolution"][0][0])
    res = face >= 0
    # every resolved wave has a one-cube signature
    assert np.all(wave[res, 1] - wave[res, 0] == 1)
    gw = sig[wave[res, 0]]
    assert np.all(geoms["type"][gw] == 1)
    lanes = pix.reshape(-1, 64)[res]
    ok = lanes != PAD
    assert np.all(ok.any(axis=1))
    key = ((lanes >> 16).astype(np.int64) * W + (lanes & 0xFFFF).astype(np.int64))[ok]
    assert len(np.unique(key)) == len(key)
    assert np.all((key // W) % count == rank)
    out = np.stack([key, np.broadcast_to(gw[:, None], lanes.shape)[ok], np.broadcast_to(face[res][:, None], lanes.shape)[ok]], axis=1)
    return out[np.argsort(out[:, 0])], int((pix != PAD).sum())


def _face_normals(geom):
    """The six world-space face normals of a cube, float64: normalize(transform (+-e_axis, 0)), face = 2 axis + (sign > 0)."""
    m = np.asarray(geom["transform"], np.float64).reshape(4, 4).T          # (column-major in the file)
    out = np.zeros((6, 3))
    for axis in range(3):
        for pos in range(2):
            v = m[:3, axis] * (1.0 if pos else -1.0)
            out[2 * axis + pos] = v / np.linalg.norm(v)
    return out


@pytest.mark.parametrize("name,W,H,floor", CASES)
def test_every_ray_of_a_resolved_pixel_enters_its_cube_through_the_certified_face(pt, oracle, name, W, H, floor):
    sc = pt.Scene(os.path.join(ROOT, "scenes", name))
    sc.set_resolution(W, H)
    cam, geoms = sc.camera.view(pt.CAMERA_DTYPE), sc.geoms.view(pt.GEOM_DTYPE)
    whole, listed = _resolved(pt, cam, geoms, 0, 1)
    share = len(whole) / max(listed, 1)
    print("%s %dx%d: %d of %d listed pixels resolved (%.3f)" % (name, W, H, len(whole), listed, share))
    if floor is not None:
        assert share >= floor                                   # (not vacuous)
    # the shards' resolved pixels together are the unsharded list's (the certificate is a property of the pixel)
    for count in (2, 3, 8):
        union = np.concatenate([_resolved(pt, cam, geoms, rank, count)[0] for rank in range(count)])
        assert np.array_equal(union[np.argsort(union[:, 0])], whole)
    if not len(whole):
        return
    sample = whole
    if len(sample) > SAMPLE:
        sample = whole[np.sort(np.random.default_rng(20240607).choice(len(whole), SAMPLE, replace=False))]
    ref = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), 1)
    L = oracle.lib()
    og = np.ascontiguousarray(sc.geoms.view(oracle.GEOM_DTYPE))
    N = len(sample)
    # rays [:, :8]: the oracle's camera rays of iterations 1..8; [:, 8:]: float32 rays through points of the unit pixel square, by the camera
    # ray's own operations (oracle camera_ray, the jitter replaced)
    f = np.float32
    rays = np.zeros((N, 16, 6), f)
    vp = C.c_void_p
    base = rays.ctypes.data
    for i, key in enumerate(sample[:, 0].tolist()):
        for it in range(1, 9):
            L.orc_camera_ray(ref.h, it, key, vp(base + 24 * (16 * i + it - 1)))
    view, up, pos = (np.asarray(cam[k][0], f) for k in ("view", "up", "position"))
    cr = np.array([view[1] * up[2] - up[1] * view[2], view[2] * up[0] - up[2] * view[0], view[0] * up[1] - up[0] * view[1]], f)
    right = cr * (f(1.0) / np.sqrt(f(cr[0] * cr[0] + cr[1] * cr[1]) + f(cr[2] * cr[2])))
    ys = f(np.tan(f(cam["fov"][0][1] * f(f(3.1415926535897932) / f(180)))))
    xs = f(f(ys * f(W)) / f(H))
    plx, ply = f(f(2.0) * xs) / f(W), f(f(2.0) * ys) / f(H)
    off = np.array([(0, 0), (1, 0), (0, 1), (1, 1), (.5, 0), (.5, 1), (0, .5), (1, .5)], f)
    px, py = (sample[:, 0] % W).astype(f), (sample[:, 0] // W).astype(f)
    a = plx * ((px[:, None] + off[None, :, 0]) - f(W * 0.5))
    b = ply * ((py[:, None] + off[None, :, 1]) - f(H * 0.5))
    d = (view[None, None, :] - right[None, None, :] * a[:, :, None]) - up[None, None, :] * b[:, :, None]
    d = d * (f(1.0) / np.sqrt((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]))[:, :, None]
    assert d.dtype == f
    rays[:, 8:, :3] = pos
    rays[:, 8:, 3:] = d
    t = np.zeros((N, 16), f)
    p = np.zeros(3, f)
    n = np.full((N, 16, 3), -7, f)
    outside = np.full((N, 16), -7, np.int32)
    nb, pb, ob, ip = n.ctypes.data, vp(p.ctypes.data), outside.ctypes.data, C.POINTER(C.c_int)
    gptr = {int(g): vp(og[int(g):int(g) + 1].ctypes.data) for g in np.unique(sample[:, 1])}
    isect = L.orc_box_intersect
    for i, g in enumerate(sample[:, 1].tolist()):
        gp = gptr[g]
        for k in range(16 * i, 16 * i + 16):
            t.flat[k] = isect(gp, vp(base + 24 * k), pb, vp(nb + 12 * k), C.cast(ob + 4 * k, ip))
    # hit, from outside, with the certified face's normal (the nearest of the cube's six, and within rounding of it)
    allN = np.stack([_face_normals(geoms[int(g)]) for g in sample[:, 1]])                   # (N, 6, 3)
    dist = np.abs(allN[:, None, :, :] - n.astype(np.float64)[:, :, None, :]).max(axis=3)     # (N, 16, 6)
    face = sample[:, 2][:, None]
    ok = (t > 0) & (outside == 1) & (dist.argmin(axis=2) == face) & (np.take_along_axis(dist, np.broadcast_to(face, (N, 16))[:, :, None], 2)[:, :, 0] < 1e-4)
    assert ok.shape == (N, 16)                                   # no ray skipped
    bad = np.argwhere(~ok)
    assert len(bad) == 0, "%d violations; first (pixel, primitive, face), ray, t, outside, n: %r" % (
        len(bad), (sample[bad[0][0]], rays[tuple(bad[0])], t[tuple(bad[0])], outside[tuple(bad[0])], n[tuple(bad[0])]))
