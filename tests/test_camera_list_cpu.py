"""The camera rays' packed work list (pt_init's build_camera_list, host code) against the row spans it is built from: for every shard
of a frame, every pixel that some primitive's span covers is listed exactly once, every wave's lanes share one signature -- the set of
primitives whose spans cover the lane's pixel -- padding lanes hold no pixel, and the listed pixels plus the ones no span covers are
the shard's pixels.  Cornell, the glass Cornell box and the 64-sphere field, at the benchmark's shapes and at the awkward ones (one
row, narrower than a wave, widths off the wave size), in shards of 1, 2, 3 and 8 members."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 0xFFFFFFFF

CASES = [
    ("cornell.txt", 1280, 720), ("cornell.txt", 1, 1), ("cornell.txt", 333, 1), ("cornell.txt", 40, 30), ("cornell.txt", 97, 61),
    ("cornell.txt", 1000, 77), ("cornell_glass.txt", 1920, 1080), ("cornell_glass.txt", 63, 200), ("spheres64.txt", 512, 512),
    ("spheres64.txt", 130, 70),
]


def _scene(pt, name, W, H):
    sc = pt.Scene(os.path.join(ROOT, "scenes", name))
    sc.set_resolution(W, H)
    return sc.camera.view(pt.CAMERA_DTYPE), sc.geoms.view(pt.GEOM_DTYPE)


def _check(pt, cam, geoms, W, H, rank, count):
    _, _, spans = pt.camera_cull_tables(cam, geoms)
    got = pt.camera_list(cam, geoms, rank, count)
    assert got is not None
    pix, wave, sig, listed, shard_px = got
    assert len(pix) % 256 == 0 and wave.shape == (len(pix) // 64, 2)
    rows = np.arange(rank, H, count)
    assert shard_px == len(rows) * W
    # the pixels the spans cover, per shard row: (row, x) -> the primitives covering it
    xs = np.arange(W)
    cover = (spans[rows, :, 0][:, None, :] <= xs[None, :, None]) & (xs[None, :, None] <= spans[rows, :, 1][:, None, :])   # (rows, W, n)
    covered = cover.any(axis=2)
    valid = pix != PAD
    assert listed == int(valid.sum()) == int(covered.sum())
    # listed exactly once, and exactly the covered pixels of the shard's rows
    x, y = (pix[valid] & 0xFFFF).astype(np.int64), (pix[valid] >> 16).astype(np.int64)
    assert np.all((y % count) == rank) and np.all(x < W) and np.all(y < H)
    key = y * W + x
    assert len(np.unique(key)) == len(key)
    want = (rows[:, None] * W + xs[None, :])[covered]
    assert np.array_equal(np.sort(key), np.sort(want))
    # every wave: one signature, exactly the primitives covering each of its lanes' pixels (file order, no duplicates)
    lane_cover = cover[(y - rank) // count, x]                                      # (listed, n)
    wv = np.nonzero(valid)[0] // 64
    for w in np.unique(wv):
        g = sig[wave[w, 0]:wave[w, 1]]
        assert len(g) > 0 and np.all(np.diff(g) > 0)
        want_sig = np.zeros(len(geoms), bool)
        want_sig[g] = True
        assert np.all(lane_cover[wv == w] == want_sig[None, :]), "wave %d holds pixels of another signature" % w
    # waves without a pixel are padding: an empty range, no valid lane
    empty = np.setdiff1d(np.arange(len(wave)), wv)
    assert np.all(~valid.reshape(-1, 64)[empty])
    return listed


@pytest.mark.parametrize("name,W,H", CASES)
def test_camera_list_covers_every_spanned_pixel_once_per_shard(pt, name, W, H):
    cam, geoms = _scene(pt, name, W, H)
    total = 0
    for count in (1, 2, 3, 8):
        per = sum(_check(pt, cam, geoms, W, H, rank, count) for rank in range(count))
        if count == 1:
            total = per
        assert per == total                                    # the shards' lists partition the unsharded one


def test_camera_list_of_the_benchmark_frame_drops_the_uncovered_pixels(pt):
    cam, geoms = _scene(pt, "cornell.txt", 1280, 720)
    pix, wave, sig, listed, shard_px = pt.camera_list(cam, geoms)
    # (not vacuous: at 16:9 a third of the frame lies outside every span, and the list is shorter than the 768-px row bands it replaces)
    assert listed < 0.8 * shard_px
    assert len(pix) < 768 * 720
