"""numpy restatement of object history (PT_FLAG_OBJECT_HISTORY; csrc/pt_temporal.h gives every operation under "MOTION", include/pt_amd.h the
host's table): the history follows primitives that moved between two views.  A composition of temporal_ref, temporal_demod_ref,
spatial_var_ref, demod_ref and denoise_var_ref, none of them edited: step 1' rewrites the guides the reprojection reads -- P', N', and a
primitive index of -1 where the row says there is no history --, steps 2 - 8 are theirs.  Every fp32 operation is one operation in the kernel's
order, the table is made in float64 with one rounding as the host makes it, so the GPU's result equals this one bit for bit.

A motion table is (n, 24) float32, a row per primitive: m[3][4] row by row, then (G[0], the bits of the int32 state), (G[1], 0), (G[2], 0);
None stands for "no table": every primitive unmoved, PT_FLAG_TEMPORAL's kernels."""
import os
import re

import numpy as np

import demod_ref as dm
import denoise_ref as dr
import denoise_var_ref as dv
import spatial_var_ref as sv
import temporal_demod_ref as td
import temporal_ref as tr

F = np.float32
UNMOVED, MOVED, NO_HISTORY = 0, 1, 2
CANDIDATE_CAPS = (4.0, 8.0, 16.0, 32.0)


def object_cap(header=None):
    """PT_OBJECT_HISTORY_MAX as include/pt_amd.h defines it"""
    header = header or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pt_amd.h")
    return F(re.search(r"^#define PT_OBJECT_HISTORY_MAX ([0-9.eE+-]+)f$", open(header).read(), re.M).group(1))


def _mat(geom, field):
    """a geom's 4 x 4 matrix as float64 M[row, column] (the record is column-major)"""
    return np.asarray(geom[field], F).reshape(4, 4).T.astype(np.float64)


def states(rows):
    return np.ascontiguousarray(np.asarray(rows, F).reshape(-1, 24)[:, 15]).view(np.int32)


def motion_table(geoms_then, geoms_now):
    """The host's table between the geoms the history's view was rendered with and the coming view's: (rows (n, 24) float32, any).
    A = T_then Tinv_now in float64, each entry ((t0 i0 + t1 i1) + t2 i2) + t3 i3; rows 0..2 rounded once: m.  G = the cofactors of A's linear
    part over its determinant (A00 c00 + A01 c01) + A02 c02, rounded once.  State 0 where transform and inverseTransform are byte-equal (the
    row then holds the identity), 2 where one of the 21 numbers is not finite, else 1.  any: a row has another state than 0."""
    a, b = np.asarray(geoms_then).reshape(-1), np.asarray(geoms_now).reshape(-1)
    assert len(a) == len(b)
    rows = np.zeros((len(a), 24), F)
    st = np.zeros(len(a), np.int32)
    for g in range(len(a)):
        if a[g]["transform"].tobytes() == b[g]["transform"].tobytes() and a[g]["inverseTransform"].tobytes() == b[g]["inverseTransform"].tobytes():
            rows[g, [0, 5, 10, 12, 17, 22]] = 1
            continue
        T, Ti = _mat(a[g], "transform"), _mat(b[g], "inverseTransform")
        with np.errstate(all="ignore"):
            A = np.empty((3, 4))
            for i in range(3):
                for j in range(4):
                    A[i, j] = ((T[i, 0] * Ti[0, j] + T[i, 1] * Ti[1, j]) + T[i, 2] * Ti[2, j]) + T[i, 3] * Ti[3, j]
            c = np.array([[A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1], A[1, 2] * A[2, 0] - A[1, 0] * A[2, 2], A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]],
                          [A[0, 2] * A[2, 1] - A[0, 1] * A[2, 2], A[0, 0] * A[2, 2] - A[0, 2] * A[2, 0], A[0, 1] * A[2, 0] - A[0, 0] * A[2, 1]],
                          [A[0, 1] * A[1, 2] - A[0, 2] * A[1, 1], A[0, 2] * A[1, 0] - A[0, 0] * A[1, 2], A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]]])
            det = (A[0, 0] * c[0, 0] + A[0, 1] * c[0, 1]) + A[0, 2] * c[0, 2]
            m, G = A.astype(F), (c / det).astype(F)
        rows[g, 0:12] = m.reshape(-1)
        rows[g, 12:15], rows[g, 16:19], rows[g, 20:23] = G[0], G[1], G[2]
        st[g] = MOVED if (np.isfinite(m).all() and np.isfinite(G).all()) else NO_HISTORY
    rows[:, 15] = st.view(F)
    return rows, bool((st != 0).any())


def history_cap(rows, header=None):
    """step 6's cap: PT_OBJECT_HISTORY_MAX under a table that holds a row of another state than 0, else PT_TEMPORAL_MAX_HISTORY"""
    if rows is None or not (states(rows) != 0).any():
        return tr.constants(header)[0]
    return object_cap(header)


def follow(pos_t, nrm_id, rows):
    """Step 1': the guides as steps 2 - 6 read them -- (pos_t', nrm_id') with P' and N' in the place of a moved primitive's P and N, t and every
    unmoved primitive's values untouched, and the primitive index -1 (step 1: no history) where the state is 2 or N' has no length.  (An index
    past the table is state 0.)"""
    pos_t, nrm_id = np.asarray(pos_t, F), np.asarray(nrm_id, F)
    if rows is None:
        return pos_t, nrm_id
    rows = np.asarray(rows, F).reshape(-1, 24)
    ids = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
    inside = (ids >= 0) & (ids < len(rows))
    r = rows[np.where(inside, ids, 0)]
    st = np.where(inside, np.ascontiguousarray(r[..., 15]).view(np.int32), 0)
    P, N = pos_t[..., :3], nrm_id[..., :3]
    with np.errstate(all="ignore"):
        Pp = np.stack([((r[..., 4 * k] * P[..., 0] + r[..., 4 * k + 1] * P[..., 1]) + r[..., 4 * k + 2] * P[..., 2]) + r[..., 4 * k + 3] for k in range(3)], axis=-1)
        g = np.stack([(r[..., 12 + 4 * k] * N[..., 0] + r[..., 13 + 4 * k] * N[..., 1]) + r[..., 14 + 4 * k] * N[..., 2] for k in range(3)], axis=-1)
        l = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
        Np = g / np.sqrt(l)[..., None]
        moved = (st == MOVED) & (l > 0)
        none = (st == NO_HISTORY) | ((st == MOVED) & ~(l > 0)) | ((st != 0) & (st != MOVED) & (st != NO_HISTORY))
    out_p, out_n = pos_t.copy(), nrm_id.copy()
    out_p[..., :3] = np.where(moved[..., None], Pp, P)
    out_n[..., :3] = np.where(moved[..., None], Np, N)
    out_n[..., 3] = np.where(none, np.int32(-1), ids).astype(np.int32).view(F)
    return out_p.astype(F), out_n.astype(F)


def _consts(rows, consts=None, cap=None):
    """temporal_ref's constants with step 6's cap in the place of the first"""
    c = tuple(consts or tr.constants())
    return (F(history_cap(rows) if cap is None else cap),) + c[1:]


def reproject(pos_t, nrm_id, hc, hn, hpos_t, hnrm_id, cam16, rows=None, consts=None, cap=None):
    """steps 1 - 6 under a table: (hc (h, w, 4), Nh (h, w))"""
    p, n = follow(pos_t, nrm_id, rows)
    return tr.reproject(p, n, hc, hn, hpos_t, hnrm_id, cam16, _consts(rows, consts, cap))


def filter_form(S, Q, n, pos_t, nrm_id, hist5, rows=None, consts=None, cap=None):
    """k_temporal<kTemporalFilter, false, MOTION>: (c, variance)"""
    p, g = follow(pos_t, nrm_id, rows)
    return tr.filter_form(S, Q, n, p, g, *hist5, consts=_consts(rows, consts, cap))


def capture_form(S, Q, n, pos_t, nrm_id, hist5, rows=None, consts=None, cap=None):
    """k_temporal<kTemporalCapture, false, MOTION>: (Hc', Hn') -- the stored count keeps PT_TEMPORAL_MAX_HISTORY"""
    c, m2, tot = tr.blend(S, Q, n, *reproject(pos_t, nrm_id, *hist5, rows=rows, consts=consts, cap=cap))
    top = (consts or tr.constants())[0]
    with np.errstate(all="ignore"):
        return np.concatenate([c, m2[..., None]], axis=2).astype(F), np.where(tot < top, tot, top).astype(F)


def moments_form(S, Q, n, pos_t, nrm_id, hist5, rows=None, consts=None, cap=None):
    """k_temporal<kTemporalMoments, false, MOTION>: (M, N), the count uncapped"""
    p, g = follow(pos_t, nrm_id, rows)
    return sv.moments_form(S, Q, n, p, g, hist5, _consts(rows, consts, cap))


def albedo_form(asum, n, pos_t, nrm_id, hist6, rows=None, consts=None, cap=None):
    """outA of every (., true, MOTION) form: (Ab, tot)"""
    p, g = follow(pos_t, nrm_id, rows)
    return td.albedo_form(asum, n, p, g, hist6, _consts(rows, consts, cap))


def capture(S, Q, n, pos_t, nrm_id, cam16, hist, rows=None, asum=None):
    """What pt_init over a live flagged renderer leaves as the context's history: the capture through the table the going renderer got at its
    own pt_init, its guides and its camera.  hist of 5 (temporal_ref's), or of 6 with asum (PT_FLAG_DEMOD_HISTORY)."""
    hc, hn = capture_form(S, Q, n, pos_t, nrm_id, hist[:5], rows)
    out = (hc, hn, np.asarray(pos_t, F), np.asarray(nrm_id, F), np.asarray(cam16, F))
    return out if asum is None else out + (albedo_form(asum, n, pos_t, nrm_id, hist, rows),)


def front(S, Q, n, pos_t, nrm_id, hist5, rows, sigma_normal, sigma_position, cap=None):
    """the image level 0 reads without demodulation: (c, v) -- the filter form from two samples on, at one (PT_FLAG_SPATIAL_VARIANCE) the moments
    form and the spatial estimate over the view's OWN guides"""
    pos_t, nrm_id = np.asarray(pos_t, F), np.asarray(nrm_id, F)
    if n >= 2:
        return filter_form(S, Q, n, pos_t, nrm_id, hist5, rows, cap=cap)
    geom = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
    M, N = moments_form(S, Q, n, pos_t, nrm_id, hist5, rows, cap=cap)
    c, v, _ = sv.spatial_variance(M, N, pos_t[..., :3], nrm_id[..., :3], geom, sv.constants()[1], sigma_normal, sigma_position)
    return c, v


def denoise_var(S, Q, n, pos_t, nrm_id, hist, rows, levels, sigma_lum, sigma_normal, sigma_position, asum=None, own_from=None, eps=dm.MIN_ALBEDO,
                cap=None):
    """pt_denoise_var of a PT_FLAG_OBJECT_HISTORY renderer whose context holds `hist` and the table `rows`: (colour (h, w, 3), variance (h, w)).
    asum given (and hist of 6): PT_FLAG_DEMOD_HISTORY's division by the blended albedo in front of the levels and the product behind them.
    cap (the study's): step 6's cap in the place of the header's."""
    pos_t, nrm_id = np.asarray(pos_t, F), np.asarray(nrm_id, F)
    geom = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
    c, v = front(S, Q, n, pos_t, nrm_id, hist[:5], rows, sigma_normal, sigma_position, cap)
    if asum is None:
        return dv.atrous_var(c, v, pos_t[..., :3], nrm_id[..., :3], geom, levels, sigma_lum, sigma_normal, sigma_position)
    ab = albedo_form(asum, n, pos_t, nrm_id, hist, rows, cap=cap)
    cd, vd = dm.demodulate(c, v, ab, 1, eps)
    co, vo = dv.atrous_var(cd, vd, pos_t[..., :3], nrm_id[..., :3], geom, levels, sigma_lum, sigma_normal, sigma_position)
    return td.remodulate(co, vo, ab, asum, n, td.min_own() if own_from is None else own_from, eps)


def display_bytes(S, Q, n, pos_t, nrm_id, hist, rows, levels, sigma_lum, sigma_normal, sigma_position, asum=None):
    """the display path's bytes of such a frame: (h * w, 4) uint8"""
    return dr.to_rgba8(denoise_var(S, Q, n, pos_t, nrm_id, hist, rows, levels, sigma_lum, sigma_normal, sigma_position, asum)[0])


def moved_geoms(oracle, geoms, moves):
    """a copy of `geoms` with the primitives of `moves` = {index: (translation, rotation, scale)} (None: as it is) posed anew, the three
    matrices by the oracle's transform builder -- the scene loader's"""
    out = np.array(geoms, copy=True)
    for g, (t, r, s) in moves.items():
        rec = out[g]
        t = rec["translation"] if t is None else t
        r = rec["rotation"] if r is None else r
        s = rec["scale"] if s is None else s
        xf, inv, it = oracle.build_transform(np.asarray(t, F), np.asarray(r, F), np.asarray(s, F))
        out["translation"][g], out["rotation"][g], out["scale"][g] = t, r, s
        out["transform"][g] = np.asarray(xf, F).reshape(-1)
        out["inverseTransform"][g] = np.asarray(inv, F).reshape(-1)
        out["invTranspose"][g] = np.asarray(it, F).reshape(-1)
    return out


def ledger(pos_t, nrm_id, hc, hn, hpos_t, hnrm_id, cam16, rows, consts=None):
    """Which branch every pixel and every tap takes under a table -- counted, not blended: a dict of pixel counts (state0, state1, state2, the
    pixels of a moved row whose N' has no length, those behind the old camera, those outside its frame) and of the taps the id, the normal and
    the plane test reject first, in the kernel's order, over the pixels of moved rows alone; `valid` (h, w): the pixels that find history."""
    cap, c_n, c_p, w_min = consts or tr.constants()
    pos_t, nrm_id = np.asarray(pos_t, F), np.asarray(nrm_id, F)
    h, w = np.asarray(hn).shape
    ids = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
    table = np.asarray(rows, F).reshape(-1, 24)
    inside = (ids >= 0) & (ids < len(table))
    st = np.where(inside, states(table)[np.where(inside, ids, 0)], -1)
    p, g = follow(pos_t, nrm_id, table)
    fid = np.ascontiguousarray(g[..., 3]).view(np.int32)
    moved = st == MOVED
    out = dict(state0=int((st == 0).sum()), state1=int(moved.sum()), state2=int((st == NO_HISTORY).sum()), no_length=int((moved & (fid < 0)).sum()))
    hids = np.ascontiguousarray(np.asarray(hnrm_id, F)[..., 3]).view(np.int32)
    with np.errstate(all="ignore"):
        s, u, v = tr.project(p[..., :3], cam16)
        live = moved & (fid >= 0)
        out["behind"] = int((live & ~(s > 0)).sum())
        inframe = (u > F(-1.0)) & (u < F(w)) & (v > F(-1.0)) & (v < F(h))
        out["outside"] = int((live & (s > 0) & ~inframe).sum())
        ok = live & (s > 0) & inframe
        x0, y0 = np.where(ok, np.floor(u), 0).astype(np.int64), np.where(ok, np.floor(v), 0).astype(np.int64)
        lim = c_p * p[..., 3]
        N, P = g[..., :3], p[..., :3]
        rej = dict(id=0, normal=0, plane=0)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                t = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                t &= np.asarray(hn, F)[cy, cx] > 0
                same = hids[cy, cx] == fid
                rej["id"] += int((t & ~same).sum())
                t &= same
                Nq, Pq = np.asarray(hnrm_id, F)[cy, cx, :3], np.asarray(hpos_t, F)[cy, cx, :3]
                near = tr._dot3(Nq[..., 0], Nq[..., 1], Nq[..., 2], N[..., 0], N[..., 1], N[..., 2]) >= c_n
                rej["normal"] += int((t & ~near).sum())
                t &= near
                off = tr._dot3(Pq[..., 0] - P[..., 0], Pq[..., 1] - P[..., 1], Pq[..., 2] - P[..., 2], N[..., 0], N[..., 1], N[..., 2])
                rej["plane"] += int((t & ~(np.abs(off) <= lim)).sum())
    out.update(("rejected_" + k, n) for k, n in rej.items())
    out["valid"] = reproject(pos_t, nrm_id, hc, hn, hpos_t, hnrm_id, cam16, table, consts)[1] > 0
    return out


# ---- the synthetic arrays of the kernel-level test -----------------------------------------------------------------------------------------
def _affine(rot_deg=(0, 0, 0), scale=(1, 1, 1), trans=(0, 0, 0)):
    """a 3 x 4 float64 map x -> R S x + t, R = Rz Ry Rx"""
    rx, ry, rz = np.radians(rot_deg)
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    return np.concatenate([Rz @ Ry @ Rx @ np.diag(np.asarray(scale, np.float64)), np.asarray(trans, np.float64)[:, None]], axis=1)


def row_of(A, state=MOVED, singular=False):
    """a table row of a 3 x 4 float64 map A: m = A rounded, G = the inverse transpose of its linear part rounded (zeros: `singular`)"""
    r = np.zeros(24, F)
    r[0:12] = np.asarray(A, np.float64).astype(F).reshape(-1)
    G = np.zeros((3, 3)) if singular else np.linalg.inv(np.asarray(A, np.float64)[:, :3]).T
    r[12:15], r[16:19], r[20:23] = G[0].astype(F), G[1].astype(F), G[2].astype(F)
    r[15] = np.array([state], np.int32).view(F)[0]
    return r


BANDS = 5
# per band of columns the motion of its three primitives: band 0 unmoved; a translation; a rotation; a non-uniform scale; and a band that
# mixes a singular G (state 1, N' without a length), a primitive without history (state 2) and all three motions at once
MOTIONS = [None, _affine(trans=(0.75, -0.5, 0.25)), _affine(rot_deg=(10, 20, -15)), _affine(scale=(1.5, 0.75, 2.0)),
           _affine(rot_deg=(-20, 5, 30), scale=(0.5, 1.25, 0.8), trans=(-1.0, 0.5, 2.0))]


def synthetic(w, h, seed):
    """test_gpu_temporal's arrays -- taps outside the frame, Hn = 0, other primitives, normal and plane rejections, NaN guides, counts on the
    cap -- under a table of 3 BANDS rows: the primitive index of a pixel, new or old, is its own 0..2 plus three times its band of columns,
    and the new view's guides of a moved band are taken through the INVERSE of its motion (float64, rounded once), so that step 1' brings them
    back next to where the generator put them.  Returns (S, Q, pos_t, nrm_id, hc, hn, hpos_t, hnrm_id, cam16, rows)."""
    from test_gpu_temporal import _synthetic
    S, Q, pos_t, nrm_id, hc, hn, hpos, hnrm_id, cam = _synthetic(w, h, seed)
    band = (np.arange(w) * BANDS // w)[None, :].repeat(h, 0)
    ids = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32).copy()
    hids = np.ascontiguousarray(hnrm_id[..., 3]).view(np.int32).copy()
    ids = np.where(ids >= 0, ids + 3 * band, ids).astype(np.int32)
    hids = np.where(hids >= 0, hids + 3 * band, hids).astype(np.int32)
    rows = np.zeros((3 * BANDS, 24), F)
    for r in range(3 * BANDS):
        b = r // 3
        if MOTIONS[b] is None:
            rows[r] = row_of(_affine(), UNMOVED)
        elif b == BANDS - 1 and r % 3 == 1:
            rows[r] = row_of(MOTIONS[b], MOVED, singular=True)
        elif b == BANDS - 1 and r % 3 == 2:
            rows[r] = row_of(MOTIONS[b], NO_HISTORY)
        else:
            rows[r] = row_of(MOTIONS[b])
    pos_t, nrm_id = pos_t.copy(), nrm_id.copy()
    with np.errstate(all="ignore"):
        for b in range(1, BANDS):
            A = MOTIONS[b]
            L, t = A[:, :3], A[:, 3]
            m = band == b
            P = pos_t[..., :3].astype(np.float64)[m]
            pos_t[..., :3][m] = ((P - t) @ np.linalg.inv(L).T).astype(F)
            N = nrm_id[..., :3].astype(np.float64)[m] @ L          # (G N ~ N_generator needs N = L^T N_generator, up to its length)
            nrm_id[..., :3][m] = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F)
    nrm_id[..., 3] = ids.view(F)
    hnrm_id = hnrm_id.copy()
    hnrm_id[..., 3] = hids.view(F)
    return S, Q, pos_t, nrm_id, hc, hn, hpos, hnrm_id, cam, rows
