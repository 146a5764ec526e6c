"""The frame plan (csrc/nrf_frame_plan.h) without a GPU: how a render call becomes launches, work queues and host-frame copies.
nrf_debug_frame_plan answers every row of tests/frame_plan_rows.py as the commit before the header existed did
(tests/golden/frame_plan_parent.json), and the answers have the properties the kernels and the copy path rely on -- each stated
here on its own terms in numpy, and each shown to fail under one deliberate mistake."""
import zlib

import numpy as np
import pytest

import frame_plan_rows as fr
import nerfhip as nh

ROWS = fr.rows()
BY_NAME = {r["name"]: r for r in ROWS}


@pytest.fixture(scope="module")
def golden():
    return fr.golden()


@pytest.fixture(scope="module")
def plans():
    return fr.plan_all(ROWS)


def test_every_row_equals_the_parent_record(golden, plans):
    assert set(golden) == set(plans)
    for name, p in plans.items():
        g = golden[name]
        if isinstance(g, list):
            assert [int(v) for v in p.flat] == g, name
        else:  # a long answer: its head field for field, its length, the crc32 of everything behind the head
            assert dict(zip(fr.HEAD, g["head"])) == p.head, name
            assert (len(p.flat), zlib.crc32(np.asarray(p.flat[24:], np.int64).tobytes())) == (g["n"], g["crc32"]), name


def test_the_record_agrees_with_the_known_figures(golden):
    """tests/test_abi_cpu.py's figures, the 24-bit refusal and either side of each bound of a planned launch"""
    head = lambda name: dict(zip(fr.HEAD, golden[name] if isinstance(golden[name], list) else golden[name]["head"]))
    assert head("geo-1920x1080-0of8")["tiles_per_shard"] == 4052 and head("geo-1920x1080-0of1")["strips"] == 8100
    assert head("geo-1920x1080-0of1")["tiles_per_shard"] == 32400 and head("geo-20x12-0of4")["tiles_per_shard"] == 4
    assert [head(f"geo-20x12-{i}of4")["local_tiles"] for i in range(4)] == [4, 4, 0, 0]  # more shards than strips
    assert head("geo-7680x4320-0of1")["views_per_launch"] == 128 and head("geo-16384x8192-0of1")["views_per_launch"] == 31
    assert (head("q-24bit-below")["n_pos"], head("q-24bit-below")["refused"]) == (0xfffffe, 0)
    assert (head("q-24bit-at")["n_pos"], head("q-24bit-at")["refused"]) == (0xffffff, 1)
    assert head("q-24bit-16384x8192")["refused"] == 1 and head("q-24bit-16384x8192-split")["refused"] == 0
    for bound in ("lds", "cap", "dil"):
        assert (head(f"q-planned-{bound}-at")["planned"], head(f"q-planned-{bound}-over")["planned"]) == (1, 0), bound
    assert head("q-planned-lds-at")["n_pos"] == 60 * 1024
    assert head("q-planned-no-buffer")["planned"] == 0 and head("q-planned-no-position")["planned"] == 0
    # the sample cap goes for one or two views that fill the chip, unless it was forced
    assert [head(f"cap-1920x1080-{n}-0")["drops_sample_cap"] for n in (1, 2, 3)] == [1, 1, 0]
    assert [head(f"cap-1920x1080-{n}-1")["drops_sample_cap"] for n in (1, 2, 3)] == [0, 0, 0]
    assert head("cap-64x48-1-0")["all_tail"] == 1 and head("cap-64x48-1-0")["drops_sample_cap"] == 0
    assert head("cap-at-the-wave-count")["all_tail"] == 0 and head("cap-below-the-wave-count")["all_tail"] == 0
    # a lone view that is planned is not progressive; without a plan, and with three views, it is
    assert head("bands-640x360-1-2-5-16384")["progressive"] == 0 and head("bands-640x360-1-2-5-0")["progressive"] == 1
    assert head("bands-640x360-3-2-5-0")["progressive"] == 1
    assert head("fill-17")["bg_u8"] == 63 and head("fill-00")["bg_u8"] == 255


def test_the_model_box_is_the_test_models():
    import grid_plan_rows as gp
    import models

    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    _, box, _ = gp.plan(desc, None, desc.mean_density, gp.ALL)
    assert tuple(float(v) for v in box) == fr.MODEL_BOX and float(desc.scale) == fr.MODEL_SCALE


# ---- 1. shards partition the frame ----
def shards_partition(W, H, world, local_tiles_of, tiles_per_shard):
    """local_tiles_of(rank) -> the rank's local tile count; returns an error string or None"""
    strips_x = ((W + 7) // 8 + 3) // 4
    total = strips_x * ((H + 7) // 8)
    seen = np.zeros(total, np.int64)
    most = 0
    for rank in range(world):
        n = local_tiles_of(rank)
        if n % 4:
            return "a strip has four tiles"
        strips = rank + world * np.arange(n // 4)
        if (strips >= total).any():
            return "a strip beyond the frame"
        seen[strips] += 1
        most = max(most, n)
        if W * H <= 640 * 360 and n != len(nh.shard_tile_ids(W, H, rank, world)):
            return "shard_tile_ids disagrees"
    if not (seen == 1).all():
        return "not every strip exactly once"
    return None if most == tiles_per_shard else "tiles_per_shard is not the largest shard"


def _geometry_cases(plans):
    for W, H in fr.SIZES:
        for world in (1, 2, 3, 4, 8):
            yield W, H, world, [plans[f"geo-{W}x{H}-{i}of{world}"].head for i in range(world)]


def test_shards_partition_the_frame(plans):
    for W, H, world, heads in _geometry_cases(plans):
        assert shards_partition(W, H, world, lambda r: heads[r]["local_tiles"], heads[0]["tiles_per_shard"]) is None, (W, H, world)
        for rank in range(world) if W * H <= 640 * 360 else ():
            ids = nh.shard_tile_ids(W, H, rank, world)
            strips_x = heads[0]["strips_x"]
            assert [ty * strips_x + tx // 4 for tx, ty in ids[::4]] == list(range(rank, heads[0]["strips"], world))


def test_mutation_a_ranks_strips_rounded_down(plans):
    def rounded_down(W, H, world):
        total = (((W + 7) // 8 + 3) // 4) * ((H + 7) // 8)
        return lambda rank: 4 * max(0, (total - rank) // world)
    broken = [(W, H, world) for W, H, world, heads in _geometry_cases(plans)
              if shards_partition(W, H, world, rounded_down(W, H, world), heads[0]["tiles_per_shard"]) is not None]
    assert broken and (8, 8, 2) in broken


# ---- 2. the region of interest is conservative ----
DEGENERATE = ("singular-pose", "nan-pose", "nan-origin", "empty-box", "org-beyond-4096", "corner-behind", "inside-the-box")


def hit_mask(W, H, cam, pose, box, scale):
    """float64: which pixel centres' rays meet the box in front of the camera (slab test)"""
    p = np.asarray(pose, np.float64).reshape(4, 4)
    ngp = p[[1, 2, 0]]  # nerf -> ngp axes (render_utils.h:68-77)
    R = ngp[:, :3] * np.array([1.0, -1.0, -1.0])
    org = ngp[:, 3] * scale
    xs = (np.arange(W) + 0.5 - float(cam[2])) / float(cam[0])
    ys = (np.arange(H) + 0.5 - float(cam[3])) / float(cam[1])
    if not all(box[a] <= box[a + 3] for a in range(3)):  # no occupied cell
        return np.zeros((H, W), bool)
    t_in, t_out = np.full((H, W), -np.inf), np.full((H, W), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(3):
            d = R[a, 0] * xs[None, :] + R[a, 1] * ys[:, None] + R[a, 2]
            t0, t1 = (box[a] - org[a]) / d, (box[a + 3] - org[a]) / d
            t_in, t_out = np.maximum(t_in, np.minimum(t0, t1)), np.minimum(t_out, np.maximum(t0, t1))
    return (t_in <= t_out) & (t_out > 0.0)


def region_is_conservative(W, H, hits, roi, rows):
    """No hitting pixel outside roi -- and none within 3 pixels of its border unless that border is the frame's: the margin
    view_roi documents (the kernel's fp32 ray directions may differ from these float64 ones by far less than a pixel; three
    are the stated reserve).  roi_rows / roi_cols cover roi."""
    x0, y0, x1, y1 = (int(v) for v in roi)
    if hits.any():
        ys, xs = np.nonzero(hits)
        if not (max(xs.min() - 3, 0) >= x0 and min(xs.max() + 3, W - 1) <= x1 and max(ys.min() - 3, 0) >= y0 and min(ys.max() + 3, H - 1) <= y1):
            return "a hitting pixel (or its margin) outside the region"
    if x1 >= x0 and y1 >= y0:
        lo, hi, c0, c1 = (int(v) for v in rows)
        if not (lo <= max(y0, 0) and min(y1, H - 1) < hi and c0 <= max(x0, 0) and min(x1, W - 1) < c1 and lo % 8 == 0 and c0 % 8 == 0):
            return "rows / columns do not cover the region"
    return None


@pytest.fixture(scope="module")
def camera_hits():
    return {"roi-" + name: (W, H, hit_mask(W, H, cam, pose, box, fr.MODEL_SCALE)) for name, W, H, cam, pose, box in fr.camera_rows()}


def test_the_region_is_conservative(golden, camera_hits):
    proper = total = 0
    for name, (W, H, hits) in camera_hits.items():
        p = fr.golden_plan(BY_NAME[name], golden)  # checked on the parent's record (which the plan equals: the first test)
        assert region_is_conservative(W, H, hits, p.roi[0], p.rows[0]) is None, name
        if not name.endswith(DEGENERATE):
            x0, y0, x1, y1 = (int(v) for v in p.roi[0])
            total += 1
            proper += hits.any() and x1 >= x0 and y1 >= y0 and (x1 - x0 + 1) * (y1 - y0 + 1) < W * H
    assert total >= 40 and 2 * proper >= total, (proper, total)  # not by every region being the whole frame
    empty = lambda name: fr.golden_plan(BY_NAME[name], golden).roi[0].tolist() == [0, 0, -1, -1]
    assert empty("roi-org-beyond-4096") and empty("roi-nan-origin") and not empty("roi-org-inside-4096")
    assert fr.golden_plan(BY_NAME["roi-empty-box"], golden).roi[0, 2:].tolist() == [-1, -1]
    for whole in ("roi-singular-pose", "roi-nan-pose", "roi-inside-the-box"):
        assert fr.golden_plan(BY_NAME[whole], golden).roi[0].tolist() == [0, 0, 639, 359], whole


def test_mutation_a_margin_of_zero(golden, camera_hits):
    broken = 0
    for name, (W, H, hits) in camera_hits.items():
        p = fr.golden_plan(BY_NAME[name], golden)
        x0, y0, x1, y1 = (int(v) for v in p.roi[0])
        shrunk = (x0 + 3 if x0 > 0 else x0, y0 + 3 if y0 > 0 else y0, x1 - 3 if x1 < W - 1 else x1, y1 - 3 if y1 < H - 1 else y1)
        broken += region_is_conservative(W, H, hits, shrunk, p.rows[0]) is not None
    assert broken >= 10


# ---- 3. the queues cover the regions, and nothing twice ----
def queues_cover(row, head, roi, queues):
    W, H, (rank, world) = row["W"], row["H"], row["shard"]
    strips_x, tiles_y = head["strips_x"], head["tiles_y"]
    local = np.arange(rank, head["strips"], world)  # the rank's strips in local order
    local_row = np.repeat(local // strips_x, 4)     # ... the strip row of each of its tiles
    begin = 0
    for v in range(head["launch_views"]):
        k_lo, k_hi, q_begin, q_rows, q_row0 = (int(x) for x in queues[v])
        y0, y1 = max(int(roi[v][1]), 0), min(int(roi[v][3]), H - 1)
        touched = set() if (roi[v][2] < roi[v][0] or y1 < y0) else set(range(y0 // 8, y1 // 8 + 1))
        if q_begin != begin or q_rows != len(touched) or (touched and q_row0 != min(touched)):
            return "the units of the views are not the touched strip rows, one after the other"
        begin += q_rows
        want = np.nonzero(np.isin(local_row, sorted(touched)))[0]
        got = np.arange(k_lo, min(k_hi, len(local_row)))
        if not np.array_equal(want, got) or k_hi < k_lo:
            return "[k_lo, k_hi) is not the rank's tiles of those rows"
    if begin != head["q_total"] or head["n_pos"] != begin * -(-strips_x // world) or not 1 <= head["n_classes"] <= 8:
        return "the total"
    return None


def _queue_rows():
    return [r for r in ROWS if r["name"].startswith("q-") and r["n_views"] <= 16]


def test_queues_cover_the_region_and_nothing_twice(plans):
    for r in _queue_rows():
        p = plans[r["name"]]
        assert queues_cover(r, p.head, p.roi, p.queues) is None, r["name"]
        assert p.head["n_classes"] == (r["classes"] if 1 <= r["classes"] <= 8 else 8)
        tiles = p.head["local_tiles"] * p.head["launch_views"]
        assert p.head["workgroups"] == max(1, min(r["n_cus"], -(-tiles // r["waves"]))) and p.head["blocks_per_view"] == p.head["local_tiles"] // 4


def test_mutation_ty1_exclusive(plans):
    broken = 0
    for r in _queue_rows():
        p = plans[r["name"]]
        q = p.queues.copy()
        q[:, 3] = np.maximum(q[:, 3] - 1, 0)  # the last strip row of every view is not queued
        q[:, 2] = np.concatenate([[0], np.cumsum(q[:, 3])[:-1]])
        head = dict(p.head, q_total=int(q[:, 3].sum()), n_pos=int(q[:, 3].sum()) * p.head["class_cols"])
        broken += queues_cover(r, head, p.roi, q) is not None
    assert broken >= len(_queue_rows()) // 2


# ---- 4. the bands tile the rows ----
def bands_tile(row, rows, bands):
    W, smallest = row["W"], (1 if row["flags"] & fr.DEPTH else 3)
    for v in range(row["n_views"]):
        lo, hi = int(rows[v][0]), int(rows[v][1])
        mine = bands[bands[:, 0] == v]
        if hi <= lo:
            if len(mine):
                return "a band of a view without rows"
            continue
        edges = [lo]
        for _, b_lo, b_hi, s0, s1 in mine.tolist():
            if b_lo != edges[-1] or b_hi <= b_lo or s0 != b_lo // 8 or s1 != (b_hi + 7) // 8:
                return "bands out of order, overlapping or empty"
            if len(mine) > 1 and (b_hi - b_lo) * W * smallest < 65536:
                return "a copy below 64 KiB"
            edges.append(b_hi)
        if edges[-1] != hi:
            return "the bands do not end with the rows"
    return None


def _band_rows(plans):
    return [r for r in ROWS if r["name"].startswith("bands-") and plans[r["name"]].head["progressive"]]


def test_bands_tile_the_rows(plans):
    several = 0
    for r in _band_rows(plans):
        p = plans[r["name"]]
        assert bands_tile(r, p.rows, p.bands) is None, r["name"]
        several += len(p.bands) > r["n_views"]
        whole = sum((int(hi) - int(lo)) * r["W"] * (4 if r["flags"] & fr.DEPTH else 3) for lo, hi in p.rows[:, :2])
        assert p.head["copied_bytes"] == whole  # whole rows of every band, both planes
    assert several >= 2  # (a lone 1080p frame has a dozen bands)


def test_mutation_a_band_remainder_dropped(plans):
    broken = 0
    for r in _band_rows(plans):
        p = plans[r["name"]]
        b = p.bands.copy()
        for v in range(r["n_views"]):
            idx = np.nonzero(b[:, 0] == v)[0]
            if len(idx):
                n = int(b[idx[-1], 4] - b[idx[0], 3]) // len(idx)  # every band n / n_bands strip rows, the remainder nobody's
                b[idx, 3] = b[idx[0], 3] + n * np.arange(len(idx))
                b[idx, 4] = b[idx, 3] + n
                b[idx, 1], b[idx, 2] = np.maximum(8 * b[idx, 3], p.rows[v][0]), np.minimum(8 * b[idx, 4], p.rows[v][1])
        broken += bands_tile(r, p.rows, b) is not None
    assert broken >= 1


# ---- 5. the fill is correct ----
MARK = 7


def replay_fills(plans, mutate=None):
    """the 40 calls on one numpy plane; returns an error string or None"""
    W, H = fr.FILL_W, fr.FILL_H
    plane = np.random.default_rng(3).integers(100, 200, (H, W)).astype(np.uint8)  # (neither a background value nor the marker)
    for i in range(40):
        p = plans[f"fill-{i:02d}"]
        bg = p.head["bg_u8"]
        f = p.fills[0]
        rects = f[1:1 + 4 * int(f[0])].reshape(-1, 4)
        if mutate:
            rects = mutate(rects, f[17:21])
        pitched, _, _, _, _, off, pitch, width, n = (int(x) for x in p.copies[0])
        off -= 3 * W * H  # the depth plane: a byte per pixel behind the rgb plane
        flat = np.zeros(W * H, bool)
        for r in range(n):
            flat[off + r * pitch:off + r * pitch + width] = True
        copied = flat.reshape(H, W)
        for r0, r1, c0, c1 in rects.tolist():
            if not (0 <= r0 < r1 <= H and 0 <= c0 < c1 <= W):
                return f"call {i}: a rectangle outside the plane, or empty"
            if copied[r0:r1, c0:c1].any():
                return f"call {i}: a fill overlaps the extent about to be copied"
            plane[r0:r1, c0:c1] = bg
        plane[copied] = MARK
        if not (plane[~copied] == bg).all():
            return f"call {i}: a pixel outside the copied extent is not the background"
        r0, r1, c0, c1 = (int(x) for x in f[17:21])
        if copied.any() and not copied[r0:r1, c0:c1].all() or copied.sum() > max(r1 - r0, 0) * (c1 - c0):
            return f"call {i}: the bookkeeping rectangle is not the copied extent"
    return None


def test_the_fill_is_correct(plans, golden):
    assert replay_fills(plans) is None
    for i in range(40):
        name = f"fill-{i:02d}"
        assert plans[name].head["fill_bytes"] <= fr.golden_plan(BY_NAME[name], golden).head["fill_bytes"], name
    # the sequence meets every case: a call that fills nothing, whole-plane fills, shared rows with columns on either side
    n_rects = [int(plans[f"fill-{i:02d}"].fills[0, 0]) for i in range(40)]
    assert 0 in n_rects and 4 in n_rects and plans["fill-17"].head["fill_bytes"] > 0


def test_mutation_the_shared_rows_columns_skipped(plans):
    def skip(rects, now):
        keep = [r for r in rects.tolist() if not (r[0] >= now[0] and r[1] <= now[1] and now[1] > now[0])]  # the rows the new rectangle has too
        return np.asarray(keep, np.int64).reshape(-1, 4)
    assert replay_fills(plans, skip) is not None
