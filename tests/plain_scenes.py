"""The PLAIN family: seeded scenes whose later bounces take k_bounce<..., PLAIN> with history-coded path pools (csrc/pt_trace.h: PathPool,
KParams::histBits), at every width of the code and at the depths at which the history word is full, nearly full, empty or one code long.

    sc, (W, H), extras, rng = plain_scene(pt, oracle, seed)          # seed: 0 .. N_SEEDS - 1

A scene is a room of up to six flat cubes (axis-aligned, some turned by whole multiples of 180 degrees, each missing with a small
probability), a ceiling light and zero to four spheres or cubes -- small ones (binned), one poking through a wall, one touching the floor,
coincident duplicates, arbitrary rotations and non-uniform scales -- over a table of `nmats` materials: material 0 emits, every third one is a
half mirror (REFL 1, exponent 0) whose specular colour is drawn apart from its colour, the rest diffuse, one of them sometimes black.  No
refractive material and no specular exponent anywhere in the table, no mesh, no texture, no direct lighting: nothing that leaves the family.

    nmats = NMATS[seed % 13]          the widths b = max(1, ceil(log2(2 nmats))) = 1, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 8, 9
    depth by DEPTH_KINDS[(seed // 13) % 5]:
        "full"       32 // b + 1: the whole word lies behind the last bounce (b = 1, 2, 4, 8: all 32 bits; else the top 32 % b bits stay unused)
        "full-1"     one less
        "one", "two" depth 1 (no history at all), depth 2 (one code)
        "between"    a random depth in between

so the 78 seeds hold every table at every kind of depth, and the full word twice.  `sc` carries what the ledger (tests/test_plain_fuzz_cpu.py)
counts: sc.nmats, sc.bits, sc.depth_kind, sc.cases (the geometric cases the generator put in) and sc.walls (the room's walls among the
primitives)."""
import types

import numpy as np

NMATS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 64, 128, 129)
DEPTH_KINDS = ("full", "full-1", "one", "two", "between")
N_SEEDS = 6 * len(NMATS)                # five kinds of depth, and the full word once more
SEED0 = 7300                            # (numpy seeds 7300 .. 7377)
TINY = 57                               # the seed with a frame of one pixel (eight materials, a depth in between)
WIDTHS, HEIGHTS = (37, 64, 96, 130), (23, 36, 50)


def code_bits(nmats):
    """history_code_bits of csrc/pt_scene_plan.h: 2 * material + (specular ? 1 : 0) < 2 nmats"""
    b = 1
    while (1 << b) < 2 * nmats:
        b += 1
    return b


def full_depth(nmats):
    """the deepest trace whose history fits one word: b * (depth - 1) <= 32"""
    return 32 // code_bits(nmats) + 1


def materials(oracle, rng, nmats):
    m = np.zeros(nmats, oracle.MATERIAL_DTYPE)
    m["color"] = rng.uniform(0.2, 1.0, (nmats, 3))
    m["emittance"][0] = rng.uniform(1, 8)
    mirrors = [i for i in range(1, nmats) if i % 3 == 2 or nmats == 2]
    for i in mirrors:                                           # half mirror, half diffuse; a swapped specular bit changes the frame
        m["hasReflective"][i], m["specColor"][i] = 1.0, rng.uniform(0.3, 1.0, 3)
    diffuse = [i for i in range(1, nmats) if i not in mirrors]
    black = None
    if len(diffuse) >= 3 and rng.random() < 0.5:
        black = int(rng.choice(diffuse))
        m["color"][black] = 0.0                                 # exactly 0: a product that stays 0 from that code on
    return m, black


def plain_scene(pt, oracle, seed):
    rng = np.random.default_rng(SEED0 + seed)
    nmats = NMATS[seed % len(NMATS)]
    bits = code_bits(nmats)
    kind = DEPTH_KINDS[(seed // len(NMATS)) % len(DEPTH_KINDS)]
    full = full_depth(nmats)
    between = int(rng.integers(3, full - 1)) if full - 2 >= 3 else min(3, full)
    depth = {"full": full, "full-1": full - 1, "one": 1, "two": 2, "between": between}[kind]
    mats, black = materials(oracle, rng, nmats)

    def surface():                                              # from all over the table, half of the draws moved to the next half mirror
        m = int(rng.integers(min(1, nmats - 1), nmats))
        mirror = m - m % 3 + 2
        return mirror if rng.random() < 0.5 and mirror < nmats else m

    def material():                                             # about one object in ten emits
        return 0 if rng.random() < 0.1 else surface()

    S = float(rng.uniform(6, 12))
    closed = kind == "full"                                     # (a full word is to be USED: a path has to reach the light behind it)
    rooms = [((0, 0, 0), (S, 0.01, S)), ((0, S, 0), (S, 0.02, S)), ((0, S / 2, -S / 2), (S, S, 0.01)),
             ((-S / 2, S / 2, 0), (0.01, S, S)), ((S / 2, S / 2, 0), (0.01, S, S)), ((0, S / 2, S / 2), (S, S, 0.01))]
    geoms, walls, cases = [], [], set()
    for k, (t, s) in enumerate(rooms):
        missing = rng.random() < 0.08
        # (not by 360 degrees: float32's sin(2 pi) is 1.7e-7, beyond what choose_walls takes for an aligned edge -- a plane wall, no PLAIN form)
        r = tuple(float(v) for v in rng.choice([0, 180, -180, 540], 3)) if rng.random() < 0.3 else (0, 0, 0)
        # (the room's surfaces do not emit; the floor takes the table's last material, the code with the highest bits)
        m = nmats - 1 if k == 0 else surface()
        if missing and not closed:
            cases.add("open")
            continue
        if any(r):
            cases.add("turned wall")
        walls.append(len(geoms))
        geoms.append(oracle.make_geom(1, m, t, r, s))
    geoms.append(oracle.make_geom(1, 0, (0, S - 0.2, 0), (0, 0, 0), (S / 2, 0.3, S / 2)))      # a large ceiling light
    # zero to four spheres or cubes (a closed room's six walls leave the light among the small cubes: three then)
    n = int(rng.integers(0, 5))
    if len(walls) == 6:
        n = min(n, 3)
    k = 0
    while k < n:
        how = str(rng.choice(["free", "small", "poke", "floor"]))
        sphere = bool(rng.random() < 0.5)
        t = np.array([rng.uniform(-0.3, 0.3) * S, rng.uniform(0.15, 0.7) * S, rng.uniform(-0.35, 0.15) * S])
        r = tuple(rng.uniform(-180, 180, 3))
        s = rng.uniform(0.8, 2.5) * rng.uniform(0.5, 1.5, 3)
        if how == "small":
            s = rng.uniform(0.15, 0.6) * rng.uniform(0.7, 1.3, 3)
        elif how == "poke":                                     # across the left or the right wall's plane, or the back wall's
            axis, side = (0, float(rng.choice([-1, 1]))) if rng.random() < 0.7 else (2, -1.0)
            t[axis] = side * S / 2 + rng.uniform(-0.2, 0.2) * s[axis]
        elif how == "floor":                                    # resting on the floor's upper face: a ball on its pole, a cube on a face
            d = float(rng.uniform(0.6, 2.0))
            s = np.array([d, d, d]) if sphere else np.array([d * rng.uniform(0.5, 1.5), d, d * rng.uniform(0.5, 1.5)])
            r = (0.0, float(rng.uniform(-180, 180)), 0.0)
            t[1] = 0.005 + s[1] / 2
        cases.add(how)
        geoms.append(oracle.make_geom(0 if sphere else 1, material(), tuple(t), r, tuple(s)))
        k += 1
        if k < n and rng.random() < 0.3:                        # coincident duplicates: file order decides
            geoms.append(geoms[-1].copy())
            if rng.random() < 0.5:
                geoms[-1]["materialid"] = material()
            cases.add("duplicate")
            k += 1
    if black is not None and len(geoms) > 2:                    # the black material on one primitive that is neither the floor nor the light
        others = [i for i in range(1, len(geoms)) if int(geoms[i]["materialid"][0]) != 0]
        geoms[int(rng.choice(others))]["materialid"] = black
    W, H = (1, 1) if seed == TINY else (int(rng.choice(WIDTHS)), int(rng.choice(HEIGHTS)))
    cam = np.zeros(1, oracle.CAMERA_DTYPE)
    cam["resolution"] = (W, H)
    # the camera stands inside the room, in front of the sixth wall
    cam["position"] = (rng.uniform(-1, 1), S / 2 + rng.uniform(-1, 1), S / 2 - 0.6)
    cam["view"], cam["up"] = (rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.05), -1), (0, 1, 0)
    cam["fov"] = (0.0, rng.uniform(30, 50))
    oracle.lib().orc_camera_set_resolution(cam.ctypes.data, W, H)
    sc = types.SimpleNamespace(geoms=np.concatenate(geoms).view(pt.GEOM_DTYPE), materials=mats.view(pt.MATERIAL_DTYPE),
                               camera=cam.view(pt.CAMERA_DTYPE), traceDepth=depth, meshes={}, mesh_normals={}, mesh_materials={},
                               image=np.zeros((H, W, 3), np.float32),
                               nmats=nmats, bits=bits, depth_kind=kind, cases=cases, walls=walls, black=black)
    extras = {}
    if rng.random() < 0.25:                                     # a thin lens: the camera-ray launch is a general form that feeds the history pool
        extras.update(lens_radius=float(rng.uniform(0.05, 0.4)), focal_distance=float(S / 2))
    return sc, (W, H), extras, rng


def oracle_renderer(oracle, sc, extras, depth=None):
    ref = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE),
                          sc.traceDepth if depth is None else depth)
    ref.set_extras(**extras)
    return ref
