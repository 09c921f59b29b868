"""The GROUPED family: seeded scenes of hundreds to thousands of swept primitives, whose later bounces take k_bounce<..., GROUPS> (csrc/pt_trace.h:
the two-level sweep, from kGroupedMin = 128 swept primitives upwards) by themselves -- PT_AMD_GROUPS is never set -- and, beside them, the flat
sweeps the older generators never plan without a mesh.

    sc, (W, H), extras, rng = grouped_scene(pt, oracle, seed)          # seed: 0 .. N_SEEDS - 1, as test_gpu_fuzz._random_scene returns them

No mesh and no texture.  A table of six materials of every kind (a light, three diffuse, a mirror with or without an exponent, glass); spheres
and small cubes at arbitrary rotations and non-uniform scales; the room's five walls present, partly missing or absent; the emitter a ceiling
light, an emissive swept sphere or both; coincident duplicates; direct lighting and a thin lens in about a fifth of the scenes each.  Frames of
48, 64 or 96 by 36 or 50 pixels, depth 2 .. 6.  sc.kind = KINDS[seed % 13] names what the seed is for:

    threshold   exactly 128 swept primitives; threshold_twin() is the same scene without its last sphere: 127, the flat sweep
    rounds      more than 1024 (up to 1100) swept primitives, an odd number: more than 128 groups, so a tile of both clusters runs THREE rounds of
                64 groups, and two clusters that the padding leaves unequal
    lds-edge    a padded table (nSphCull) of exactly 1280 entries -- the last one staged in LDS -- or 1288, the first one read from global memory
    global      1400 .. 2200 swept primitives: level 2 from global memory; every other one with swept cubes
    onion       200 .. 400 spheres around one point, radii spread over a decade, half of them glass: a ray through the middle is a candidate of
                every group, and a lane's column of kCandPairs = 12 parked words fills up
    cubes       130 .. 300 swept primitives, three in four of them cubes, some of those thin plates seen edge-on
    open        no walls; three in four hold an ellipsoid flat beyond the culling's reach, so build_sphere_clusters gives up (n0 == 0)
    swept       5 .. 127 swept primitives, no mesh: cubes among them, a lens, or both -- many|sweptCubes, dof|many, dof|many|sweptCubes

A swept primitive is a sphere, or a cube that is neither binned (the four smallest) nor a wall (the six largest): the generator asks the plan
(pt.sphere_groups) how many a scene has and drops spheres off its tail until the count is the one it wants.  sc.nswept is that count; sc.cases
what the generator put in; sc.emitter "light", "sphere" or "both"."""
import types

import numpy as np

KINDS = ("threshold", "rounds", "lds-edge", "global", "global", "onion", "onion", "cubes", "cubes", "open", "swept", "swept", "swept")
N_SEEDS = 4 * len(KINDS)                # four of every column: 8 global, onion, cubes; 12 swept; 4 of the others
SEED0 = 9100                            # (numpy seeds 9100 .. 9151)
WIDTHS, HEIGHTS = (48, 64, 96), (36, 50)
LDS_EDGE = (1280, 1288, 1280, 1288)     # nSphCull of the four lds-edge scenes
FULL_COLUMN = (5, 6, 44)                      # the three onion scenes whose oracle paths pass 24 groups or more (the ledger checks it)
EMIT_MAX = 8                            # kEmitMax of csrc/pt_trace.h
TAIL = 12                               # spheres at the end of every list: what the count is adjusted with


def _material(oracle, rng, kind):
    m = np.zeros(1, oracle.MATERIAL_DTYPE)
    m["color"] = rng.uniform(0.2, 1.0, 3)
    if kind == "light":
        m["emittance"] = rng.uniform(2, 8)
    elif kind == "mirror":
        m["hasReflective"], m["specColor"] = 1.0, rng.uniform(0.5, 1.0, 3)
        m["specExponent"] = rng.choice([0.0, 0.0, 5.0, 300.0])
    elif kind == "glass":
        m["hasRefractive"], m["indexOfRefraction"], m["specColor"] = 1.0, rng.choice([1.33, 1.5, 2.4]), rng.uniform(0.7, 1.0, 3)
    return m


def plan_options(pt, extras):
    """the extras of a scene as pt.scene_plan / pt.sphere_groups take them"""
    o = {k: v for k, v in extras.items() if k != "direct_lighting"}
    if extras.get("direct_lighting"):
        o["flags"] = pt.PT_FLAG_DIRECT_LIGHTING
    return o


def _assemble(pt, oracle, head, prims, mats, cam, depth, **attrs):
    geoms = np.concatenate(head + prims)
    W, H = (int(v) for v in cam["resolution"][0])
    return types.SimpleNamespace(geoms=geoms.view(pt.GEOM_DTYPE), materials=mats.view(pt.MATERIAL_DTYPE), camera=cam.view(pt.CAMERA_DTYPE),
                                 traceDepth=depth, meshes={}, mesh_normals={}, mesh_materials={}, image=np.zeros((H, W, 3), np.float32), **attrs)


def grouped_scene(pt, oracle, seed):
    rng = np.random.default_rng(SEED0 + seed)
    kind, variant = KINDS[seed % len(KINDS)], seed // len(KINDS)
    mats = np.concatenate([_material(oracle, rng, k) for k in ["light", "diffuse", "diffuse", "mirror", "glass", "diffuse"]])
    cases = set()
    S = float(rng.uniform(8, 14))
    centre = np.array([0, S / 2, 0])

    # ---- the room and the emitter
    head = []
    walls = {"open": "absent"}.get(kind, str(rng.choice(["present", "present", "partly", "absent"])))
    if walls != "absent":
        room = [((0, 0, 0), (S, 0.01, S)), ((0, S, 0), (S, 0.01, S)), ((0, S / 2, -S / 2), (S, S, 0.01)),
                ((-S / 2, S / 2, 0), (0.01, S, S)), ((S / 2, S / 2, 0), (0.01, S, S))]
        for t, s in room:
            if walls == "partly" and rng.random() < 0.4:
                continue
            head.append(oracle.make_geom(1, int(rng.integers(1, 6)), t, (0, 0, 0), s))
    cases.add("walls " + walls)
    emitter = str(rng.choice(["sphere", "both"] if kind == "onion" else ["light", "sphere", "both"]))
    if emitter != "sphere":
        head.append(oracle.make_geom(1, 0, (0, S - 0.2, 0), (0, 0, 0), (S / 3, 0.3, S / 3)))

    # ---- how many swept primitives, and of which sort
    lens = bool(rng.random() < 0.2)
    cube_share = 0.0
    if kind == "threshold":
        target, cube_share = 128, (0.0, 0.3, 0.0, 0.5)[variant]
    elif kind == "rounds":
        target, cube_share = 1025 + 2 * int(rng.integers(0, 38)), (0.0, 0.2, 0.0, 0.0)[variant]
    elif kind == "lds-edge":
        target = LDS_EDGE[variant]                              # (the search below lowers it until the padded table has this size)
    elif kind == "global":
        target, cube_share = int(rng.integers(1400, 2201)), 0.25 * (seed % 2)
        lens = False                                            # (a lens on so large a table: lens_global_scene, which the plan may refuse)
    elif kind == "onion":
        target = int(rng.integers(200, 401))
    elif kind == "cubes":
        target, cube_share = int(rng.integers(130, 301)), 0.75
    elif kind == "open":
        target, cube_share = int(rng.integers(130, 501)), 0.2 * (variant % 2)
    else:
        # the flat sweeps without a mesh: column 10 cubes and no lens, column 11 a lens and no swept cube, column 12 both
        column = seed % len(KINDS)
        target = int(rng.choice([5, 6, 17, 40, 90, 127] if column == 11 else [17, 40, 90, 127])) if variant else (127, 5, 64)[column - 10]
        cube_share, lens = (0.6, 0.0, 0.6)[column - 10], column != 10

    # ---- the primitives: `target` + 10 of them (ten cubes at the most are binned or walls), and behind them TAIL spheres
    n = (target if kind == "lds-edge" else target + 10 + TAIL)
    ext = rng.uniform(0.3, 0.45, 3) * S * np.where(rng.random(3) < 0.3, 0.4, 1.0)          # (sometimes a slab or a column)
    base = rng.uniform(0.2, 0.5) * S / n ** (1 / 3)
    radii = 0.04 * S * 10 ** rng.uniform(0, 1, n) if kind == "onion" else None            # 0.04 S .. 0.4 S
    spread = (0.01, 0.03, 0.1, 0.02)[variant] * S
    prims = []
    for k in range(n):
        tail = k >= n - TAIL
        cube = (not tail) and bool(rng.random() < cube_share)
        t = centre + rng.uniform(-1, 1, 3) * ext
        r = tuple(rng.uniform(-180, 180, 3))
        d = base * rng.uniform(0.6, 1.4)
        s = np.array([d, d, d]) if rng.random() < 0.5 else d * rng.uniform(0.6, 1.5, 3)
        mat = int(rng.integers(1, 6))
        if kind == "onion":
            t = centre + rng.normal(size=3) * spread
            s = radii[k] * (np.ones(3) if rng.random() < 0.7 else rng.uniform(0.8, 1.2, 3))
            mat = 4 if rng.random() < 0.5 else (0 if rng.random() < 0.12 else mat)     # (half glass; a few shells glow: light at every depth of the onion)
        elif cube and rng.random() < 0.2:                       # a thin plate, level with the camera: its edge faces the eye
            s = np.array([d * 2, d * 2 * rng.uniform(0.025, 0.05), d * 2])
            r = (0.0, float(rng.uniform(-180, 180)), 0.0)
            t[1] = S / 2 + rng.uniform(-0.3, 0.3)
            cases.add("plate")
        prims.append(oracle.make_geom(1 if cube else 0, mat, tuple(t), r, tuple(s)))
        if not tail and k + 1 < n - TAIL and rng.random() < 0.02:       # coincident duplicates: file order decides
            prims.append(prims[-1].copy())
            if rng.random() < 0.5:
                prims[-1]["materialid"] = int(rng.integers(1, 6))
            cases.add("duplicate")
    del prims[n - TAIL:len(prims) - TAIL]                       # (the duplicates came on top: the list keeps its length and its tail)
    if emitter != "light":                                      # an emissive swept sphere, larger than its neighbours; in the open a lamp
        big = (0.5 * S, 0.08 * S, 0.5 * S) if kind == "open" else tuple(max(rng.uniform(3.0, 6.0) * base, 0.08 * S) * np.ones(3))
        at = centre + np.array([0, 0.42 * S, 0]) if kind == "open" else centre + rng.uniform(-1, 1, 3) * ext
        if kind == "onion":                                     # the onion's core
            big, at = tuple(0.1 * S * np.ones(3)), centre
        prims[0] = oracle.make_geom(0, 0, tuple(at), tuple(rng.uniform(-20, 20, 3)), big)
    if emitter == "sphere" and kind != "onion":                 # ... and two more of its neighbours glow
        prims[2]["materialid"] = prims[3]["materialid"] = 0
    # flat beyond the culling's reach (aspect 100): no clusters for this scene (the last lds-edge scene: 161 groups in one stretch)
    if (kind == "open" and variant != 3) or (kind == "lds-edge" and variant == 3):
        prims[1] = oracle.make_geom(0, int(rng.integers(1, 6)), tuple(centre + rng.uniform(-0.2, 0.2, 3) * S), tuple(rng.uniform(-180, 180, 3)),
                                    (0.2 * S, 0.002 * S, 0.15 * S))
        cases.add("never culled")

    # ---- the camera, in front of the room's open side
    W, H = int(rng.choice(WIDTHS)), int(rng.choice(HEIGHTS))
    if kind == "global":                                        # (the oracle's time is the test's: the largest tables in the smallest frame)
        W, H = WIDTHS[0], HEIGHTS[0]
    cam = np.zeros(1, oracle.CAMERA_DTYPE)
    cam["resolution"] = (W, H)
    cam["position"] = (rng.uniform(-1, 1), S / 2 + rng.uniform(-1, 1), S * 1.05)
    cam["view"], cam["up"] = (rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.05), -1), (0, 1, 0)
    if kind == "onion":                                         # at the middle of the onion
        cam["view"] = tuple(centre - cam["position"][0])
    cam["fov"] = (0.0, rng.uniform(30, 45))
    oracle.lib().orc_camera_set_resolution(cam.ctypes.data, W, H)
    depth = int(rng.integers(4, 7)) if kind == "onion" else int(rng.integers(2, 7))
    extras = {}
    if lens:
        extras.update(lens_radius=float(rng.uniform(0.05, 0.4)), focal_distance=float(S * 1.05))
    if rng.random() < 0.2:
        extras.update(direct_lighting=True)

    if extras.get("direct_lighting"):                           # (the direct-lighting bounce chooses among eight emitters at the most: pt_init refuses more)
        glowing = [g for g in head + prims if int(g["materialid"][0]) == 0]
        for g in glowing[EMIT_MAX:]:
            g["materialid"] = 5
        cases.add("direct lighting, %s emitters" % ("eight" if len(glowing) >= EMIT_MAX else "fewer"))

    # ---- the count: spheres off the tail until the plan sweeps `target` primitives (lds-edge: until its padded table has that size)
    def build(m):
        sc = _assemble(pt, oracle, head, prims[:m], mats, cam, depth, kind=kind, variant=variant, cases=cases, emitter=emitter, walls=walls)
        g = pt.sphere_groups(sc, **plan_options(pt, extras))
        sc.nswept = g.nswept
        return sc, g
    m = len(prims)
    sc, g = build(m)
    size = (lambda g: len(g.table)) if kind == "lds-edge" else (lambda g: g.nswept)
    while size(g) > target and m > 1:
        over = size(g) - target
        m -= over if kind != "lds-edge" and m - over >= len(prims) - TAIL else 1      # (a sphere of the tail less is a swept primitive less)
        sc, g = build(m)
    assert size(g) == target, (seed, kind, size(g), target)
    return sc, (W, H), extras, rng


def threshold_twin(pt, sc):
    """a threshold scene without its last primitive, a sphere: 127 swept primitives, the flat sweep"""
    geoms = sc.geoms[:-1].copy()
    return types.SimpleNamespace(**{**vars(sc), "geoms": geoms, "nswept": sc.nswept - 1, "kind": "threshold twin"})


def lens_global_scene(pt, oracle, count, cubes):
    """A scene of `count` swept primitives -- a quarter of them cubes where `cubes` -- under a thin lens: its camera-ray launch takes the flat MANY
    [CUBES] DOF form over the grouped plan's tables, which plan_lds may refuse for LDS.  -> (scene, (W, H), extras); the scene is not planned here."""
    rng = np.random.default_rng(SEED0 + 1000 + count + (1 if cubes else 0))
    mats = np.concatenate([_material(oracle, rng, k) for k in ["light", "diffuse", "diffuse", "mirror", "glass", "diffuse"]])
    S = 10.0
    head = [oracle.make_geom(1, 1, (0, 0, 0), (0, 0, 0), (S, 0.01, S)), oracle.make_geom(1, 0, (0, S - 0.2, 0), (0, 0, 0), (S / 3, 0.3, S / 3))]
    base = 0.35 * S / count ** (1 / 3)
    prims = []
    n = count + TAIL + (10 if cubes else 0)                     # (as grouped_scene counts: the last TAIL of them spheres)
    for k in range(n):
        cube = cubes and k < n - TAIL and rng.random() < 0.25
        t = np.array([0, S / 2, 0]) + rng.uniform(-1, 1, 3) * 0.4 * S
        d = base * rng.uniform(0.6, 1.4)
        prims.append(oracle.make_geom(1 if cube else 0, int(rng.integers(1, 6)), tuple(t), tuple(rng.uniform(-180, 180, 3)), (d, d, d)))
    cam = np.zeros(1, oracle.CAMERA_DTYPE)
    cam["resolution"] = (48, 36)
    cam["position"], cam["view"], cam["up"] = (0, S / 2, S * 1.05), (0, 0, -1), (0, 1, 0)
    cam["fov"] = (0.0, 40.0)
    oracle.lib().orc_camera_set_resolution(cam.ctypes.data, 48, 36)
    extras = dict(lens_radius=0.2, focal_distance=float(S * 1.05))
    m = len(prims)
    while True:
        sc = _assemble(pt, oracle, head, prims[:m], mats, cam, 3, kind="lens", cases=set())
        sc.nswept = pt.sphere_groups(sc, **extras).nswept
        if sc.nswept <= count:
            break
        m -= sc.nswept - count
    assert sc.nswept == count, (count, cubes, sc.nswept)
    return sc, (48, 36), extras
