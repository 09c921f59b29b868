"""Albedo demodulation (PT_FLAG_DEMODULATE) on the MI355X, every comparison bit for bit: k_albedo's increment of a single iteration against the
colour the renderer's own path carries after its first bounce (debug_trace_paths), batches against single calls, pt_denoise_var and the display
path against the numpy restatement (tests/demod_ref.py + tests/denoise_var_ref.py), that nothing else moves, and the quality on the device's
own frames of a textured wall.  Frames: 37 x 23 and 130 x 70 (widths off the wave, partial tiles) and 64 x 8 (smaller than the step-16
stencil)."""
import os
import subprocess
import types

import numpy as np
import pytest

import demod_ref as dm
import denoise_ref as dr
import denoise_var_ref as dv
import spatial_var_ref as sv
import temporal_ref as tr
from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu
F = np.float32
FRAMES = [(37, 23), (130, 70), (64, 8)]
LENS = dict(lens_radius=0.3, focal_distance=10.0)
DEPTH = 4
EXE = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rmse(a, ref):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - ref) ** 2)))


# ---- the scene -------------------------------------------------------------------------------------------------------------------------------
def wall_texture():
    """66 x 66 texels in cells of 19: the back wall's face is 22.6 pixels wide at 130 x 70 (the camera's half height is tan(45 degrees) per unit of
    distance, the wall 15.5 units away and 10 wide: 2.26 pixels per unit), so a cell is 6.5 pixels.  Cells alternate between a dark and a light
    random colour; two are black."""
    rng = np.random.default_rng(41)
    n = 4
    dark, light = rng.uniform(0.15, 0.35, (n, n, 3)), rng.uniform(0.6, 0.95, (n, n, 3))
    iy, ix = np.mgrid[0:n, 0:n]
    cells = np.where(((ix + iy) % 2 == 0)[..., None], dark, light)
    cells[1, 1] = cells[2, 3] = 0.0
    return np.repeat(np.repeat(cells, 19, 0), 19, 1)[:66, :66].astype(F).copy()


def cell_colours(seed):
    return np.random.default_rng(seed).uniform(0.2, 1.0, (4, 4, 3)).astype(F)


def cell_texture(seed):
    return np.repeat(np.repeat(cell_colours(seed), 8, 0), 8, 1).copy()


def build(pt, orc, w, h):
    """One scene for every test: the Cornell walls with the textured back wall, a textured sphere and a textured cube, a UV-mapped mesh two of
    whose four faces have materials of their own (one diffuse, one emissive), a mirror sphere, a glass sphere and the light."""
    cam = pt.Scene(os.path.join(SCENES, "cornell.txt"))
    cam.set_resolution(w, h)
    m = np.zeros(7, pt.MATERIAL_DTYPE)
    rows = [((1, 1, 1), (0, 0, 0), 0, 0, 0, 5),                     # 0 the light
            ((.98, .98, .98), (0, 0, 0), 0, 0, 0, 0),               # 1 diffuse white
            ((.85, .35, .35), (0, 0, 0), 0, 0, 0, 0),               # 2 diffuse red
            ((.35, .85, .35), (0, 0, 0), 0, 0, 0, 0),               # 3 diffuse green
            ((.9, .95, .8), (.97, .9, .85), 1, 0, 0, 0),            # 4 a mirror
            ((.95, .9, .98), (.92, .96, .9), 0, 1, 1.5, 0),         # 5 glass
            ((.3, .4, .9), (0, 0, 0), 0, 0, 0, 0)]                  # 6 diffuse blue: a mesh face's own
    for i, (col, spec, refl, refr, ior, emit) in enumerate(rows):
        m[i] = (col, 0, spec, refl, refr, ior, emit)
    g = [orc.make_geom(1, 0, (0, 10, 0), (0, 0, 0), (3, .3, 3)),                    # 0 the light
         orc.make_geom(1, 1, (0, 0, 0), (0, 0, 0), (10, .01, 10)),                  # 1 floor
         orc.make_geom(1, 1, (0, 10, 0), (0, 0, 90), (.01, 10, 10)),                # 2 ceiling
         orc.make_geom(1, 1, (0, 5, -5), (0, 90, 0), (.01, 10, 10)),                # 3 the back wall: the cell texture
         orc.make_geom(1, 2, (-5, 5, 0), (0, 0, 0), (.01, 10, 10)),                 # 4 left
         orc.make_geom(1, 3, (5, 5, 0), (0, 0, 0), (.01, 10, 10)),                  # 5 right
         orc.make_geom(0, 1, (-2.6, 2.0, 0.5), (20, 40, 10), (3.0, 2.6, 2.8)),      # 6 a textured sphere
         orc.make_geom(1, 1, (2.6, 1.8, 0.0), (15, 30, 10), (2.2, 3.4, 2.0)),       # 7 a textured cube
         orc.make_geom(0, 4, (-2.8, 7.0, -2.0), (0, 0, 0), (2.4, 2.4, 2.4)),        # 8 a mirror sphere
         orc.make_geom(0, 5, (2.4, 6.6, 1.0), (0, 0, 0), (2.2, 2.2, 2.2))]          # 9 a glass sphere
    # 10 the mesh: a strip of two quads in its xy plane, UVs affine over the strip; faces 0, 1 the object's material, 2 its own, 3 emissive
    q = lambda x0, x1: [[x0, -.5, 0, x1, -.5, 0, x1, .5, 0], [x0, -.5, 0, x1, .5, 0, x0, .5, 0]]
    tris = np.array(q(-1.0, 0.0) + q(0.0, 1.0), F)
    xy = tris.reshape(4, 3, 3)[:, :, :2].astype(np.float64)
    uvs = np.stack([0.05 + 0.45 * (xy[..., 0] + 1.0), 0.1 + 0.8 * (xy[..., 1] + 0.5)], -1).reshape(4, 6).astype(F)
    g.append(orc.make_geom(2, 1, (0.2, 4.6, -2.5), (-10, 15, 8), (3.0, 2.6, 1)))
    geoms = np.concatenate(g).view(pt.GEOM_DTYPE)
    textures = [wall_texture(), cell_texture(5), cell_texture(6), cell_texture(7)]
    gt = np.full(len(geoms), -1, np.int32)
    gt[3], gt[6], gt[7], gt[10] = 0, 1, 2, 3
    return types.SimpleNamespace(geoms=geoms, materials=m, camera=cam.camera.copy(), traceDepth=DEPTH, meshes={10: tris}, mesh_normals={},
                                 mesh_materials={10: np.array([-1, -1, 6, 0], np.int32)}, mesh_uvs={10: uvs}, textures=textures, geom_textures=gt,
                                 geom_bumps=None, bump_scales=None, image=np.zeros((h, w, 3), F))


@pytest.fixture(scope="module")
def scenes(gpu, oracle):
    return {wh: build(gpu, oracle, *wh) for wh in FRAMES}


def _init(pt, sc, demod=True, **opts):
    opts.setdefault("max_batch", 8)
    pt.pathtraceFree()
    pt.pathtraceInit(sc, traceDepth=DEPTH, moments=True, demodulate=demod, **opts)


def _guides(pt, w, h, guide_iter=1):
    pos_t, nrm, geom = pt.gbuffer(guide_iter)
    return pos_t[:, :3].reshape(h, w, 3), nrm.reshape(h, w, 3), geom.reshape(h, w)


def _state(pt, w, h):
    """(S, Q, the guides of iteration 1) of the current renderer"""
    return pt.readback(w * h).reshape(h, w, 3), pt.readback_moments().reshape(h, w), _guides(pt, w, h)


@pytest.fixture(scope="module")
def albedo4(gpu, scenes):
    """the albedo sums of iterations 1..4 per frame, by the test library's renderer (the kernels of the product, its own instance): what the
    tests of the product library's results divide by.  test_increment_* pins them from outside."""
    out = {}
    with gpu.renderer_from_test_library():
        for (w, h), sc in scenes.items():
            _init(gpu, sc)
            gpu.pathtrace_batch(None, 0, 1, 4)
            out[(w, h)] = gpu.test_albedo().reshape(h, w, 4)
    return out


# ---- A_i pinned from outside ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,opts", [(130, 70, {}), (130, 70, LENS), (130, 70, dict(direct_lighting=True)), (37, 23, {}), (64, 8, LENS)],
                         ids=["130x70", "130x70-lens", "130x70-direct", "37x23", "64x8-lens"])
def test_increment_is_the_colour_the_path_carries_after_its_first_bounce(gpu, scenes, w, h, opts):
    sc = scenes[(w, h)]
    ones = np.ones(3, F)
    mats, geoms = sc.materials, sc.geoms
    seen = dict(diffuse=0, textured=0, own_face=0, ones=0, black=0)
    # inside a cell of the mesh's texture the face with a material of its own carries that material's colour times the cell's, to the bit
    own = (mats["color"][6][None, :] * cell_colours(7).reshape(16, 3)).astype(F)
    with gpu.renderer_from_test_library():
        for it in (1, 2, 3, 4):
            _init(gpu, sc, **opts)
            o, d, col, pix = gpu.debug_trace_paths(it, 1, w * h)
            _init(gpu, sc, **opts)
            gpu.pathtrace(None, 0, it, readback=False)
            a = gpu.test_albedo()
            geom = gpu.gbuffer(it)[2]
            assert (a[:, 3] == 1).all()
            alive = np.zeros(w * h, bool)
            alive[pix] = True
            colour = np.ones((w * h, 3), F)
            colour[pix] = col
            hit = geom >= 0
            mat = mats[geoms["materialid"][np.maximum(geom, 0)]]
            special = (mat["emittance"] > 0) | (mat["hasReflective"] > 0) | (mat["hasRefractive"] > 0)
            mesh = hit & (geoms["type"][np.maximum(geom, 0)] == 2)
            # a primitive with one material: the rule is decided by the guides' primitive; a diffuse first hit leaves a live path
            plain = hit & ~mesh & ~special
            assert alive[plain].all()
            assert _same(a[plain, :3], colour[plain])
            rest = ~hit | (hit & ~mesh & special)
            assert (a[rest, :3] == ones).all()
            # the mesh: its faces are diffuse (a live path, the object's material or the face's own) or emissive (the path ends there)
            assert _same(a[mesh & alive, :3], colour[mesh & alive]) and (a[mesh & ~alive, :3] == ones).all()
            seen["diffuse"] += int(plain.sum())
            seen["textured"] += int((plain & (sc.geom_textures[np.maximum(geom, 0)] >= 0)).sum())
            seen["own_face"] += int((mesh & alive & (a[:, None, :3] == own[None]).all(axis=2).any(axis=1)).sum())
            seen["ones"] += int((a[:, :3] == ones).all(axis=1).sum())
            seen["black"] += int((plain & (a[:, :3] == 0).all(axis=1)).sum())
    print("%d x %d %s: %s" % (w, h, opts, seen))
    assert seen["diffuse"] and seen["textured"] and seen["ones"]
    if (w, h) == (130, 70):
        assert seen["own_face"] and seen["black"]


@pytest.mark.parametrize("w,h", FRAMES)
def test_a_batch_equals_its_single_calls(gpu, scenes, w, h):
    sc = scenes[(w, h)]
    with gpu.renderer_from_test_library():
        _init(gpu, sc)
        for it in range(1, 6):
            gpu.pathtrace(None, 0, it, readback=False)
        single = gpu.test_albedo()
        S = gpu.readback(w * h)
        assert (single[:, 3] == 5).all()
        for depth in (1, 3):
            _init(gpu, sc, pipeline_depth=depth, max_batch=8)
            gpu.pathtrace_batch(None, 0, 1, 5)
            assert _same(gpu.test_albedo(), single) and _same(gpu.readback(w * h), S)
        _init(gpu, sc, pipeline_depth=3, max_batch=2)
        _, done = gpu.iterate_until(1, 1e-6, 5, check_every=2)
        assert done == 5 and _same(gpu.test_albedo(), single) and _same(gpu.readback(w * h), S)
        # two batches: the sums go on where they were
        _init(gpu, sc, max_batch=8)
        gpu.pathtrace_batch(None, 0, 1, 2)
        gpu.pathtrace_batch(None, 0, 3, 3)
        assert _same(gpu.test_albedo(), single)


# ---- the filter's result -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", FRAMES)
def test_denoise_var_under_the_flag_is_the_restatement(gpu, scenes, albedo4, w, h):
    sc, asum = scenes[(w, h)], albedo4[(w, h)]
    _init(gpu, sc)
    gpu.pathtrace_batch(None, 0, 1, 4)
    S, Q, g = _state(gpu, w, h)
    assert (asum[..., 3] == 4).all() and (asum[..., :3] < 4).any()
    for levels in (1, 3, 5):
        want, wantv = dm.denoise_var_demod(S, Q, asum, 4, *g, levels, 4.0, 0.35, 2.0)
        assert np.isfinite(want).all()
        got, gotv = gpu.denoise_var(4, levels=levels, with_variance=True)
        assert _same(got, want) and _same(gotv, wantv), levels
        assert _same(gpu.denoise_var(4, levels=levels), want)
        assert np.array_equal(gpu.denoise_var_rgba8(4, levels=levels), dr.to_rgba8(want))
    # other parameters, another guide iteration
    g2 = _guides(gpu, w, h, 3)
    want, wantv = dm.denoise_var_demod(S, Q, asum, 4, *g2, 2, 2.0, 0.5, 1.0)
    got, gotv = gpu.denoise_var(4, levels=2, sigma_lum=2.0, sigma_normal=0.5, sigma_position=1.0, guide_iter=3, with_variance=True)
    assert _same(got, want) and _same(gotv, wantv)
    # the demodulated filter is not the plain one here
    assert not _same(dv.denoise_var(S, Q, 4, *g, 5, 4.0, 0.35, 2.0)[0], dm.denoise_var_demod(S, Q, asum, 4, *g, 5, 4.0, 0.35, 2.0)[0])
    gpu.pathtraceFree()


@pytest.mark.parametrize("w,h", FRAMES)
def test_every_form_of_the_levels(gpu, scenes, w, h):
    """every level in the gather and the two tiled shapes (the last one AtrousDemod's): through the renderer, and -- k_demodulate's two forms,
    the last level's packed and BYTES stores -- over host arrays"""
    sc = scenes[(w, h)]
    with gpu.renderer_from_test_library():
        _init(gpu, sc)
        gpu.pathtrace_batch(None, 0, 1, 4)
        asum = gpu.test_albedo().reshape(h, w, 4)
        S, Q, g = _state(gpu, w, h)
        pos_t, nrm_id = tr.pack_guides(*gpu.gbuffer(1), h, w)
        want = {levels: dm.denoise_var_demod(S, Q, asum, 4, *g, levels, 4.0, 0.35, 2.0) for levels in (1, 3, 5)}
        for form in (0, 1, 2, 3):
            for levels in (1, 3, 5):
                got, gotv = gpu.test_denoise_var(4, form, levels=levels)
                assert _same(got, want[levels][0]) and _same(gotv, want[levels][1]), (form, levels)
    c, v = dv.mean_and_variance(S, Q, 4)
    cd, vd = dm.demodulate(c, v, asum, 4)
    img = np.concatenate([c, v[..., None]], axis=2)
    # sums the renderer does not produce: a zero, a NaN, a huge one
    odd = asum.copy()
    odd[0, 0, :3], odd[h - 1, w - 1, :3], odd[h // 2, w // 2, :3] = 0.0, np.nan, 1e30
    for form in (1, 2, 3):
        for levels in (1, 3):
            r = gpu.test_demodulate(form, w, h, 4, levels, asum, pos_t, nrm_id, rgb_sum=S, lum_sq_sum=Q)
            assert _same(r["demod"][:, :3], cd) and _same(r["demod"][:, 3], vd)
            assert _same(r["rgb"], want[levels][0]) and _same(r["var"], want[levels][1]), (form, levels)
            r = gpu.test_demodulate(form, w, h, 4, levels, asum, pos_t, nrm_id, rgb_sum=S, lum_sq_sum=Q, want_var=False)
            assert _same(r["rgb"], want[levels][0]) and r["var"] is None
            r = gpu.test_demodulate(form, w, h, 4, levels, asum, pos_t, nrm_id, rgb_sum=S, lum_sq_sum=Q, bytes_out=True)
            assert np.array_equal(r["rgba"], dr.to_rgba8(want[levels][0]))
            # in place on an image: the same operations on what it holds
            r = gpu.test_demodulate(form, w, h, 4, levels, asum, pos_t, nrm_id, img=img)
            assert _same(r["demod"][:, :3], cd) and _same(r["demod"][:, 3], vd) and _same(r["rgb"], want[levels][0]) and _same(r["var"], want[levels][1])
        wo, wov = dm.denoise_var_demod(S, Q, odd, 4, *g, 3, 4.0, 0.35, 2.0)
        r = gpu.test_demodulate(form, w, h, 4, 3, odd, pos_t, nrm_id, rgb_sum=S, lum_sq_sum=Q)
        assert _same(r["rgb"], wo) and _same(r["var"], wov)


@pytest.mark.parametrize("w,h", FRAMES)
def test_one_sample_under_the_spatial_variance_estimate(gpu, scenes, w, h):
    sc = scenes[(w, h)]
    with gpu.renderer_from_test_library():
        _init(gpu, sc, spatial_variance=True)
        gpu.pathtrace(None, 0, 1, readback=False)
        asum = gpu.test_albedo().reshape(h, w, 4)
        S, Q, g = _state(gpu, w, h)
        M, N = sv.moments_form(S, Q, 1)
        c, v, est = sv.spatial_variance(M, N, *g, gpu.PT_SPATIAL_RADIUS, 0.35, 2.0)
        assert est.all()
        for levels in (1, 5):
            want, wantv = dm.atrous_demod(c, v, asum, 1, *g, levels, 4.0, 0.35, 2.0)
            got, gotv = gpu.denoise_var(1, levels=levels, with_variance=True)
            assert _same(got, want) and _same(gotv, wantv), levels
        # from two samples on: the accumulators' form
        gpu.pathtrace(None, 0, 2, readback=False)
        asum = gpu.test_albedo().reshape(h, w, 4)
        S, Q, g = _state(gpu, w, h)
        assert _same(gpu.denoise_var(2), dm.denoise_var_demod(S, Q, asum, 2, *g, 5, 4.0, 0.35, 2.0)[0])


def _pbo(w, h):
    import torch
    t = torch.full((w * h, 4), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("w,h", FRAMES)
def test_the_display_path_shows_the_demodulated_filter(gpu, scenes, albedo4, w, h):
    sc, asum = scenes[(w, h)], albedo4[(w, h)]
    pbo = _pbo(w, h)
    try:
        _init(gpu, sc, display_filter=True)
        gpu.pathtrace_batch(pbo.data_ptr(), 0, 1, 4)
        gpu.sync()
        shown = pbo.cpu().numpy()
        S, Q, g = _state(gpu, w, h)
        bytes_ = dr.to_rgba8(dm.denoise_var_demod(S, Q, asum, 4, *_guides(gpu, w, h, gpu.PT_DISPLAY_GUIDE_ITER), gpu.PT_DISPLAY_LEVELS, gpu.PT_DISPLAY_SIGMA_LUM,
                                                  gpu.PT_DISPLAY_SIGMA_NORMAL, gpu.PT_DISPLAY_SIGMA_POSITION)[0])
        assert np.array_equal(shown, bytes_)
        assert np.array_equal(gpu.readback_rgba8(4, w * h), bytes_) and np.array_equal(gpu.denoise_var_rgba8(4), bytes_)
        assert not np.array_equal(bytes_, dr.to_rgba8(dv.denoise_var(S, Q, 4, *g, 5, 4.0, 0.35, 2.0)[0]))
    finally:
        gpu.pathtraceFree()
        del pbo


# ---- nothing else moves --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(130, 70), (37, 23)])
def test_everything_else_is_the_unflagged_renderer(gpu, scenes, w, h):
    sc = scenes[(w, h)]
    res = []
    for demod in (False, True):
        _init(gpu, sc, demod=demod, pipeline_depth=2, max_batch=4)
        gpu.pathtrace_batch(None, 0, 1, 4)
        gpu.pathtrace(None, 0, 5, readback=False)
        st = gpu.noise_stats(5, 0.05, tile_map=True)
        res.append(dict(S=gpu.readback(w * h), Q=gpu.readback_moments(), var=gpu.variance(5), tile=st.pop("tile_rel_var"), stats=st,
                        plain=gpu.denoise(5), pos=gpu.gbuffer(2)[0], nrm=gpu.gbuffer(2)[1], geom=gpu.gbuffer(2)[2], bytes=gpu.readback_rgba8(5, w * h),
                        dvar=gpu.denoise_var(5)))
    off, on = res
    for k in ("S", "Q", "var", "tile", "plain", "pos", "nrm"):
        assert _same(off[k], on[k]), k
    assert np.array_equal(off["geom"], on["geom"]) and np.array_equal(off["bytes"], on["bytes"]) and off["stats"] == on["stats"]
    g = (off["pos"], off["nrm"], off["geom"])
    g1 = _guides(gpu, w, h, 1)
    want = dv.denoise_var(off["S"].reshape(h, w, 3), off["Q"].reshape(h, w), 5, *g1, 5, 4.0, 0.35, 2.0)[0]
    assert _same(off["dvar"], want) and not _same(on["dvar"], want)
    gpu.pathtraceFree()


# ---- quality on the device's own frames ----------------------------------------------------------------------------------------------------
def test_the_textured_wall_is_closer_to_the_converged_frame(gpu, scenes, albedo4):
    """130 x 70, 4 samples against the mean of 1024: on the textured back wall the demodulated filter's RMSE is below the plain variance-guided
    filter's; the whole frame's is printed.  Measured: the wall's 229 pixels 0.3310 unfiltered, 0.2014 variance-guided, 0.1932 demodulated; the
    frame 0.2022 / 0.0875 / 0.0874 (most of it is flat-coloured or a miss).  (No ratio is fixed: the footprints of real pixels on the cells were never measured; the values
    printed here are the README's.)"""
    w, h = 130, 70
    sc = scenes[(w, h)]
    _init(gpu, sc, max_batch=64)
    gpu.pathtrace_batch(None, 0, 1, 4)
    flagged = gpu.denoise_var(4).reshape(h, w, 3)
    raw = gpu.readback(w * h).reshape(h, w, 3) / F(4)
    wall = gpu.gbuffer(1)[2].reshape(h, w) == 3
    for first in range(5, 1025, 64):
        gpu.pathtrace_batch(None, 0, first, min(64, 1025 - first))
    truth = (gpu.readback(w * h).reshape(h, w, 3) / F(1024)).astype(np.float64)
    _init(gpu, sc, demod=False)
    gpu.pathtrace_batch(None, 0, 1, 4)
    plain = gpu.denoise_var(4).reshape(h, w, 3)
    gpu.pathtraceFree()
    rows = [("frame", np.ones((h, w), bool)), ("textured wall", wall)]
    for name, m in rows:
        print("%-14s (%4d pixels) RMSE at 4 samples: unfiltered %.4f  variance-guided %.4f  demodulated %.4f" % (
            name, int(m.sum()), _rmse(raw[m], truth[m]), _rmse(plain[m], truth[m]), _rmse(flagged[m], truth[m])))
    assert wall.sum() > 200
    assert _rmse(flagged[wall], truth[wall]) < _rmse(plain[wall], truth[wall])


# ---- pt_render and the shim ------------------------------------------------------------------------------------------------------------------
def test_pt_render_and_the_shims_switch(gpu, tmp_path):
    """pt_render --denoise-var .. --demodulate -- through the shim one iteration per call, through the C ABI with --batch -- and the shim's
    PT_AMD_DEMODULATE=1 write the demodulated filter's frame; the usual image stays the raw mean.  (--batch on Cornell: that path of the
    driver registers no textures.)"""
    from test_host import _decode_png
    W, H = 64, 48
    env = dict(os.environ)
    for k in ("PT_AMD_DEVICES", "PT_AMD_DISPLAY_FILTER", "PT_AMD_SPATIAL_VARIANCE", "PT_AMD_DEMODULATE"):
        env.pop(k, None)
    conv = lambda m: (np.clip(m, 0, 1) * F(255)).astype(np.uint8)[:, ::-1]          # the driver's PNG conversion, X mirrored
    cases = {"cornell_textured.txt": {"plain": ([], env), "flag": (["--demodulate"], env), "shim": ([], dict(env, PT_AMD_DEMODULATE="1"))},
             "cornell.txt": {"plain": ([], env), "batch": (["--demodulate", "--batch", "4"], env)}}
    for scene, runs in cases.items():
        args = [EXE, os.path.join(SCENES, scene), "--res", str(W), str(H), "--iterations", "4", "--depth", "4", "--denoise-var", "5", "4.0", "0.35", "2.0"]
        for name, (extra, e) in runs.items():
            r = subprocess.run(args + extra + ["--out", str(tmp_path / (scene + name))], capture_output=True, text=True, timeout=120, env=e)
            assert r.returncode == 0, (scene, name, r.stderr[-2000:])
        sc = gpu.Scene(os.path.join(SCENES, scene))
        sc.set_resolution(W, H)
        mean = {}
        try:
            for demod in (False, True):
                _init(gpu, sc, demod=demod, max_batch=4)
                gpu.pathtrace_batch(None, 0, 1, 4)
                frame = gpu.readback(W * H).reshape(H, W, 3) / F(4)
                mean[demod] = gpu.denoise_var(4, 5, 4.0, 0.35, 2.0).reshape(H, W, 3)
        finally:
            gpu.pathtraceFree()
        assert not np.array_equal(conv(mean[True]), conv(mean[False])), scene
        for name in runs:
            assert np.array_equal(_decode_png(str(tmp_path / (scene + name + ".png"))), conv(frame)), (scene, name)
            assert np.array_equal(_decode_png(str(tmp_path / (scene + name + ".denoised.png"))), conv(mean[name != "plain"])), (scene, name)
