"""Adaptive sampling (include/pbrhip.h "adaptive sampling") in numpy: the per-pixel error in float32 with every operation
rounded once, the tile error as the float64 butterfly over xor distances 1 .. 32, the stop rule, the stable compaction and the level
schedule.  `run` is driven by a callback that returns PLAIN full frames at given levels: the contract says an adaptive layer is made of
such frames, pixel by pixel."""
import numpy as np

TILE = 8
CANONICAL_NAN = np.uint32(0x7FC00000)


def tiles_across(n):
    return -(-int(n) // TILE)


def levels(first_level, max_sample):
    """n_0 = min(first_level, max), n_k = min(2 n_{k-1}, max): the last level is max whatever its ratio to the one before"""
    out = [min(int(first_level), int(max_sample))]
    while out[-1] < max_sample:
        out.append(min(2 * out[-1], int(max_sample)))
    return out


def tile_box(tile, width, height):
    """x0, y0, clipped width, clipped height of tile id ty * ceil(W / 8) + tx"""
    across = tiles_across(width)
    x0, y0 = (int(tile) % across) * TILE, (int(tile) // across) * TILE
    return x0, y0, min(TILE, width - x0), min(TILE, height - y0)


def tile_pixels(tile, width, height):
    """the tile's pixels y * W + x, row-major"""
    x0, y0, cw, ch = tile_box(tile, width, height)
    ys, xs = np.mgrid[y0:y0 + ch, x0:x0 + cw]
    return (ys * width + xs).astype(np.uint32).reshape(-1)


def pixel_error(rgba, snapshot, n_prev, n_now):
    """e per pixel (H, W) float32: a = A / n_prev, b = (I - A) / (n_now - n_prev), m = I / n_now, d = |a - b| summed r, g, b left to
    right, s = m.r + m.g + m.b, e = d / sqrt(s + 1e-3f)"""
    f = np.float32
    I, A = np.asarray(rgba, f)[..., :3], np.asarray(snapshot, f)[..., :3]
    with np.errstate(all="ignore"):
        a = A / f(n_prev)
        b = (I - A) / f(n_now - n_prev)
        m = I / f(n_now)
        d = np.abs(a - b)
        d = (d[..., 0] + d[..., 1]) + d[..., 2]
        s = (m[..., 0] + m[..., 1]) + m[..., 2]
        e = d / np.sqrt(s + f(1e-3))
    assert e.dtype == f
    return e


def tile_error(e, tile, width, height):
    """E (float64): lane (y & 7) * 8 + (x & 7), absent lanes 0, v <- v + v[lane ^ o] for o = 1, 2, 4, 8, 16, 32, lane 0 / pixel count"""
    x0, y0, cw, ch = tile_box(tile, width, height)
    v = np.zeros((TILE, TILE), np.float64)
    v[:ch, :cw] = e[y0:y0 + ch, x0:x0 + cw].astype(np.float64)
    v = v.reshape(64)
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for o in (1, 2, 4, 8, 16, 32):
            v = v + v[lane ^ o]
        return v[0] / np.float64(cw * ch)


def stored_error(E):
    """(float)E as tile_error stores it: a NaN as the canonical quiet NaN"""
    with np.errstate(all="ignore"):
        out = np.float32(E)
    return CANONICAL_NAN.view(np.float32) if np.isnan(out) else out


def step(rgba, snapshot, n_prev, n_now, threshold, tiles_in, tile_error_inout=None):
    """One decision step.  Returns (tiles_out, pixels_out, tile_error, new_snapshot): the tiles with not (E <= threshold) in the order
    they had, their pixels tile after tile, the error image (entries of tiles not in tiles_in as given, else 0), and the snapshot with
    A = I for the pixels of tiles_in."""
    rgba = np.asarray(rgba, np.float32)
    h, w = rgba.shape[:2]
    snap = np.array(snapshot, np.float32, copy=True).reshape(h, w, 4)
    err = np.zeros(tiles_across(h) * tiles_across(w), np.float32) if tile_error_inout is None else np.array(tile_error_inout, np.float32, copy=True).reshape(-1)
    e = pixel_error(rgba, snap, n_prev, n_now)
    thr = np.float64(np.float32(threshold))
    tiles_out, pixels_out = [], []
    for t in np.asarray(tiles_in, np.uint32).reshape(-1):
        E = tile_error(e, t, w, h)
        err[t] = stored_error(E)
        if not (E <= thr):  # a NaN compares false: the tile stays active
            tiles_out.append(t)
            pixels_out.append(tile_pixels(t, w, h))
        x0, y0, cw, ch = tile_box(t, w, h)
        snap[y0:y0 + ch, x0:x0 + cw] = rgba[y0:y0 + ch, x0:x0 + cw]
    pixels_out = np.concatenate(pixels_out) if pixels_out else np.zeros(0, np.uint32)
    return np.asarray(tiles_out, np.uint32), pixels_out.astype(np.uint32), err.reshape(tiles_across(h), tiles_across(w)), snap


def rank_tiles(width, height, tile_rank=0, tile_world=1, shard_block=0):
    """the tiles of a rank (block index % world == rank), in image order -- no result depends on the order"""
    block = shard_block or 64
    assert block % TILE == 0
    across_b = -(-width // block)
    out = []
    for t in range(tiles_across(width) * tiles_across(height)):
        x0, y0, _, _ = tile_box(t, width, height)
        if ((y0 // block) * across_b + x0 // block) % tile_world == tile_rank:
            out.append(t)
    return np.asarray(out, np.uint32)


def run(frame_at, width, height, max_sample, threshold, first_level=8, tiles=None):
    """The whole schedule over plain frames: frame_at(n) -> (rgba (H, W, 4) float32, count (H, W)) of a plain render of n passes.
    Returns dict(rgba, count, tile_error, samples, rounds, levels): what RenderAdaptive must return, bit for bit."""
    lv = levels(first_level or 8, max_sample)
    active = rank_tiles(width, height) if tiles is None else np.asarray(tiles, np.uint32)
    th, tw = tiles_across(height), tiles_across(width)
    err = np.zeros((th, tw), np.float32)
    level_of = np.zeros((th, tw), np.int64)  # the level each tile holds
    if len(active) == 0:
        z = np.zeros((height, width, 4), np.float32)
        return dict(rgba=z, count=np.zeros((height, width), np.uint32), tile_error=err, samples=0, rounds=0, levels=lv)
    level_of.reshape(-1)[active] = lv[0]
    snap, rounds = frame_at(lv[0])[0], 1
    for k in range(1, len(lv)):
        if len(active) == 0:
            break
        level_of.reshape(-1)[active] = lv[k]
        rounds += 1
        # the layer at this point: every tile at its own level; only the active tiles (all at lv[k]) are read by the step
        I = frame_at(lv[k])[0]
        active, _, err, snap = step(I, snap, lv[k - 1], lv[k], threshold, active, err)
    rgba = np.zeros((height, width, 4), np.float32)
    count = np.zeros((height, width), np.uint32)
    for n in np.unique(level_of):
        if n == 0:
            continue
        fr, fc = frame_at(int(n))
        mask = np.kron(level_of == n, np.ones((TILE, TILE), bool))[:height, :width]
        rgba[mask], count[mask] = fr[mask], fc[mask]
    return dict(rgba=rgba, count=count, tile_error=err, samples=int(count.astype(np.int64).sum()), rounds=rounds, levels=lv)
