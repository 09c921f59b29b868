"""The later bounces' wall-face certificate (csrc/pt_device.h: wallFaceCertificate), without a GPU: its numpy float32 restatement against the
numpy float32 restatement of the reference's slab loop (tests/wall_face_ref.py), on Cornell's five walls and on one wall turned by 90 degrees
about each axis (float32 transforms that are not exactly axis-aligned), 2^18 seeded rays per wall.

(a) soundness: wherever the certificate accepts, the loop returns a hit, from outside, through the certified face -- no violation;
(b) not vacuous: every ray -- the handful with NaN, inf and zero components aside, which the certificate refuses by design -- whose float64
    hit point lies inside the face shrunk by 1 % of its side is accepted (the certificate's margins are 2^-12 relative and 2^-16 absolute);
(c) the plan's per-wall faces (pt_test_wall_faces): the expected face for each Cornell wall, -1 for the light and the sphere, -1 everywhere
    under PT_AMD_NO_WALL_RESOLVE=1."""
import numpy as np
import pytest

import wall_face_ref as ref

RAYS = 1 << 18

# scenes/cornell.txt: the floor (object 1, thin in y, below the room) is entered through its +y face, 2 * 1 + 1; the ceiling (object 2: thin
# in object x, turned by 90 degrees about z, so object +x is world +y) through its -x face; the back wall (object 3: thin in object x, turned by 90 degrees
# about y, so object +x is world -z) through its -x face; the left wall (x = -5) through +x, the right wall (x = +5) through -x
CORNELL_FACES = {0: -1, 1: 3, 2: 0, 3: 0, 4: 1, 5: 0, 6: -1}


@pytest.fixture(scope="module")
def scenes(pt):
    out = []
    for name, sc, walls in ref.load_scenes(pt):
        face, beyond = pt.wall_faces(sc)
        out.append((name, sc, walls, face, beyond))
    return out


def test_the_plan_names_the_inner_face_of_every_cornell_wall(pt, scenes, monkeypatch):
    name, sc, walls, face, beyond = scenes[0]
    assert {i: int(f) for i, f in enumerate(face)} == CORNELL_FACES
    assert all(beyond[i] > 0.5 for i in walls) and beyond[0] == 0 and beyond[6] == 0
    # the turned walls keep a face: the one whose outward normal points into the room
    for name, sc, walls, face, beyond in scenes[1:]:
        for g in walls:
            assert face[g] >= 0, name
            inv, xf = ref.matrices(sc.geoms.view(pt.GEOM_DTYPE)[g])
            K, s = int(face[g]) >> 1, (1.0 if face[g] & 1 else -1.0)
            centre = xf.astype(np.float64)[:3, :3] @ (np.eye(3)[K] * 0.5 * s) + xf.astype(np.float64)[:3, 3]
            normal = s * inv.astype(np.float64)[K, :3]
            assert np.dot(normal, np.array([0.0, 5.0, 0.0]) - centre) > 0, name
    monkeypatch.setenv("PT_AMD_NO_WALL_RESOLVE", "1")
    off, _ = pt.wall_faces(scenes[0][1])
    assert np.all(off == -1)


def test_the_certificate_is_sound_and_not_vacuous(pt, scenes):
    total = accepted = 0
    for name, sc, walls, face, beyond in scenes:
        geoms = sc.geoms.view(pt.GEOM_DTYPE)
        room = ref.room_box(geoms, [1, 2, 3, 4, 5])
        for g in walls:
            f = int(face[g])
            assert f >= 0
            org, dirs, special = ref.rays_for_wall(geoms[g], f, room, RAYS, seed=20250 + 16 * g + len(name))
            inv, _ = ref.matrices(geoms[g])
            qo, qdu = ref.to_object_space(inv, org, dirs)
            ok = ref.certificate(qo, qdu, f, beyond[g])
            hit, outside, lface, _ = ref.slab_loop(qo, qdu)
            # (a) soundness
            bad = np.nonzero(ok & ~(hit & outside & (lface == f)))[0]
            assert len(bad) == 0, "%s, object %d: %d violations; first ray %r %r" % (name, g, len(bad), org[bad[0]], dirs[bad[0]])
            assert not np.any(ok & special & ~np.isfinite(qdu).all(axis=1))
            # (b) not vacuous
            must = ref.hit_inside_shrunk_face(geoms[g], f, org, dirs) & ~special
            missed = np.nonzero(must & ~ok)[0]
            assert len(missed) == 0, "%s, object %d: %d rays inside the shrunk face refused; first %r %r" % (name, g, len(missed), org[missed[0]], dirs[missed[0]])
            assert must.sum() > RAYS // 8                       # (the family itself is not vacuous)
            total += RAYS
            accepted += int(ok.sum())
            print("%s, object %d face %d: accepted %d of %d, inside the shrunk face %d" % (name, g, f, int(ok.sum()), RAYS, int(must.sum())))
    assert accepted > total // 8
