"""The rows of tests/test_frame_plan_cpu.py and test_frame_plan_gpu.py: the inputs of one render call -- frame size, shard, views
(cameras, or regions of interest given directly), device and context figures -- and a loader of nrf_debug_frame_plan.
tests/golden/frame_plan_parent.json holds, per row, what the commit BEFORE nrf_frame_plan.h existed decided for those inputs.  That
commit had no entry point for any of it: the record was made on a CPU from a scratch copy of it whose nrf_api.hip had a recorder
appended behind nrf_debug_frame_plan's signature -- view_roi, roi_rows, roi_cols, local_tiles, nrf_tiles_per_shard and host_quant_u8
called unchanged, the inline blocks (launch_render's queues, the per-launch / all-tail / progressive rules, the band loop, copy_rows'
extents, the fill) lifted verbatim with only their inputs renamed -- and this module's record() run against that library."""
import ctypes as C
import json
import zlib
from pathlib import Path

import numpy as np

import nerfhip as nh
import synthetic as syn

GOLDEN = Path(__file__).resolve().parent / "golden" / "frame_plan_parent.json"
HEAD = ("tiles_x", "tiles_y", "strips_x", "strips", "local_tiles", "tiles_per_shard", "views_per_launch", "all_tail", "drops_sample_cap",
        "progressive", "launch_views", "q_total", "n_classes", "class_cols", "workgroups", "blocks_per_view", "refused", "planned", "n_pos",
        "copied_bytes", "n_bands", "n_fill", "fill_bytes", "bg_u8")
FORCED, DEPTH, COLS, PROGRESSIVE, HAVE_PLAN, ALL_BG, ONE_LAUNCH, HOST = 1, 2, 4, 8, 16, 32, 64, 128
RENDER_WAVES = 4  # (csrc/nrf_render.h)
N_CUS, PERSIST_WAVES = 256, 16  # an MI355X, the hot shape's workgroup
PLAN_MAX_POS = 1 << 14  # (nrf_context::plan_max_pos)
# the occupied box and the pose scale of models.build_model(log2_hashmap_size=12, H=32), the model of the GPU tests (test_frame_plan_cpu.py
# compares it with nrf_debug_grid_plan's)
MODEL_BOX = (-0.5625, -0.5, -0.4375, 0.6875, 0.4375, 0.4375)
MODEL_SCALE = 0.33000001311302185
SIZES = ((8, 8), (20, 12), (36, 20), (101, 77), (333, 211), (640, 360), (1920, 1080), (7680, 4320))


def _row(name, W, H, shard=(0, 1), cams=None, poses=None, rois=None, flags=0, classes=0, n_cus=N_CUS, waves=PERSIST_WAVES, plan_max_pos=PLAN_MAX_POS,
         plan_cap=PLAN_MAX_POS, dil_bytes=2048, prev=(0, 0, 0, 0), prev_from=None, box=MODEL_BOX, scale=MODEL_SCALE, bg=1.0):
    n = len(rois) if rois is not None else len(cams)
    return dict(name=name, W=W, H=H, shard=shard, cams=cams, poses=poses, rois=rois, n_views=n, flags=flags, classes=classes, n_cus=n_cus, waves=waves,
                plan_max_pos=plan_max_pos, plan_cap=plan_cap, dil_bytes=dil_bytes, prev=prev, prev_from=prev_from, box=box, scale=scale, bg=bg)


def away(pose):
    m = pose.copy()
    m[:3, 0] *= -1.0
    m[:3, 2] *= -1.0
    return m


def region(kind, W, H, k=0):
    """a region of interest given directly: the whole frame, none, one strip row, rows cut by the frame's edges"""
    ty = (H + 7) // 8
    if kind == "full":
        return (0, 0, W - 1, H - 1)
    if kind == "empty":
        return (0, 0, -1, -1)
    if kind == "row":
        r = k % ty
        return (0, 8 * r, W - 1, min(8 * r + 7, H - 1))
    if kind == "cut-low":  # partly negative
        return (-3, -9, W // 2, H // 3)
    assert kind == "cut-high"  # beyond the frame
    return (W // 4, H // 2, W + 20, H + 9)


KINDS = ("full", "empty", "row", "cut-low", "cut-high")


def _geometry_rows():
    out = []
    for W, H in SIZES + ((16384, 8192), (8, 1 << 20)):
        for n in (1, 2, 3, 4, 8):
            for i in range(n):
                out.append(_row(f"geo-{W}x{H}-{i}of{n}", W, H, (i, n), rois=[region("full", W, H)]))
    return out


def camera_rows():
    """(name, W, H, cam, pose, box): one view each"""
    out = []
    for W, H in ((640, 360), (101, 77)):
        base = syn.default_camera(W, H)
        for r, rn in ((3.0, "3"), (4.03, "4.03"), (9.0, "9"), (14.0 / 0.33, "14by0.33")):
            for az, el in ((40, 20), (130, -35), (250, 60), (10, 5)):
                out.append((f"orbit-{W}x{H}-r{rn}-az{az}-el{el}", W, H, base, syn.orbit_pose(az, el, radius=r), MODEL_BOX))
    W, H = 640, 360
    base = syn.default_camera(W, H)
    far, near = syn.orbit_pose(40, 20, radius=14.0 / 0.33), syn.orbit_pose(40, 20, radius=3.0 / 0.33)
    for i, (dx, dy, pose) in enumerate(((-200, 0, far), (200, 0, far), (0, 0, near), (0, -100, far), (250, 120, far), (0, 0, away(far)), (-250, -120, far),
                                        (0, 0, syn.orbit_pose(10, 40)), (120, 60, far))):
        cam = base.copy()
        cam[2] += dx
        cam[3] += dy
        out.append((f"shift-{i}", W, H, cam, pose, MODEL_BOX))
    out.append(("inside-the-box", W, H, base, syn.orbit_pose(30, 10, radius=0.3), MODEL_BOX))
    out.append(("corner-behind", W, H, base, syn.orbit_pose(50, 20, radius=0.4 / 0.33), MODEL_BOX))
    singular, nan = syn.orbit_pose(30, 30), syn.orbit_pose(30, 30)
    singular[:3, 1] = singular[:3, 0]
    nan[1, 2] = np.nan
    out.append(("singular-pose", W, H, base, singular, MODEL_BOX))
    out.append(("nan-pose", W, H, base, nan, MODEL_BOX))
    out.append(("nan-origin", W, H, base, np.where(np.arange(16).reshape(4, 4) == 7, np.float32(np.nan), syn.orbit_pose(30, 30)).astype(np.float32), MODEL_BOX))
    out.append(("empty-box", W, H, base, syn.orbit_pose(30, 30), (1.0, 1.0, 1.0, -1.0, -1.0, -1.0)))
    out.append(("org-inside-4096", W, H, base, syn.orbit_pose(30, 30, radius=4095.5 / MODEL_SCALE), MODEL_BOX))
    out.append(("org-beyond-4096", W, H, base, syn.orbit_pose(30, 30, radius=4096.5 / MODEL_SCALE), MODEL_BOX))
    return out


def _region_rows():
    return [_row("roi-" + name, W, H, cams=[cam], poses=[pose], box=box, flags=HOST | DEPTH | COLS | PROGRESSIVE | HAVE_PLAN)
            for name, W, H, cam, pose, box in camera_rows()]


def _queue_rows():
    out = []
    k = 0
    for W, H in SIZES:
        for N in (1, 2, 3):
            for i in range(N):
                for kind in KINDS:
                    out.append(_row(f"q-{W}x{H}-{i}of{N}-1-{kind}", W, H, (i, N), rois=[region(kind, W, H, k)], classes=(0, 1, 8, 9)[k % 4], flags=HAVE_PLAN))
                    k += 1
                for n in (2, 3, 16, 128):  # the views take the kinds in turn, from another one in every row
                    rois = [region(KINDS[(v + k) % len(KINDS)], W, H, v + k) for v in range(n)]
                    out.append(_row(f"q-{W}x{H}-{i}of{N}-{n}", W, H, (i, N), rois=rois, classes=(0, 1, 8, 9)[k % 4], flags=HAVE_PLAN))
                    k += 1
    # the 24-bit refusal (one launch of 128 views, whatever views_per_launch says): 8 pixels wide, a position per strip row
    W, H = 8, 1 << 20
    ty = H // 8
    for name, last in (("below", ty - 2), ("at", ty - 1)):  # 0xfffffe positions, 0xffffff
        out.append(_row(f"q-24bit-{name}", W, H, rois=[region("full", W, H)] * 127 + [(0, 0, W - 1, 8 * last - 1)], flags=ONE_LAUNCH))
    out.append(_row("q-24bit-16384x8192", 16384, 8192, rois=[region("full", 16384, 8192)] * 32, flags=ONE_LAUNCH))
    out.append(_row("q-24bit-16384x8192-split", 16384, 8192, rois=[region("full", 16384, 8192)] * 32))
    # planned or not: either side of the buffer's capacity, of the positions' LDS bound and of the dilated table's
    W, H = 8, 4096  # 512 strip rows per view, a position each: 120 views are 60 * 1024 positions
    full = [region("full", W, H)] * 120
    one = [region("row", W, H, 3)]
    for name, rois, cap, dil, flags in (("lds-at", full, 1 << 20, 2048, HAVE_PLAN), ("lds-over", full + one, 1 << 20, 2048, HAVE_PLAN),
                                        ("cap-at", full[:3], 3 * 512, 2048, HAVE_PLAN), ("cap-over", full[:3] + one, 3 * 512, 2048, HAVE_PLAN),
                                        ("dil-at", full[:3], 1 << 14, 60 * 1024, HAVE_PLAN), ("dil-over", full[:3], 1 << 14, 60 * 1024 + 4, HAVE_PLAN),
                                        ("no-buffer", full[:3], 1 << 14, 2048, 0), ("no-position", [region("empty", W, H)] * 2, 1 << 14, 2048, HAVE_PLAN)):
        out.append(_row("q-planned-" + name, W, H, rois=rois, plan_cap=cap, dil_bytes=dil, flags=flags))
    # the sample cap: few tiles (all tail), one / two / three views, forced
    for W, H in ((64, 48), (1920, 1080)):
        for n in (1, 2, 3):
            for forced in (0, FORCED):
                out.append(_row(f"cap-{W}x{H}-{n}-{forced}", W, H, rois=[region("full", W, H)] * n, flags=forced))
    out.append(_row("cap-at-the-wave-count", 1024, 256, rois=[region("full", 1024, 256)]))  # 32 x 32 tiles = 256 CUs x 4 waves
    out.append(_row("cap-below-the-wave-count", 1024, 256, rois=[region("full", 1024, 256)], waves=5))
    return out


def _band_rows():
    out = []
    for W, H in ((96, 56), (640, 360), (1920, 1080)):
        ty = (H + 7) // 8
        for n in (1, 3, 16):
            for depth in (DEPTH, 0):
                for rows in (1, 5, ty) + {135: (100,), 45: (40,)}.get(ty, ()):  # (... and counts that leave the bands a remainder)
                    rois = [(0, 8 * ((v + 1) % (ty - rows + 1)), W - 1, min(H - 1, 8 * ((v + 1) % (ty - rows + 1)) + 8 * rows - 1)) for v in range(n)]
                    for pm in (0, PLAN_MAX_POS):  # (a lone view that is planned is not progressive)
                        if pm and n > 1:
                            continue
                        out.append(_row(f"bands-{W}x{H}-{n}-{depth}-{rows}-{pm}", W, H, rois=rois, flags=HOST | PROGRESSIVE | COLS | depth, plan_max_pos=pm, plan_cap=pm))
    return out


FILL_W, FILL_H = 96, 56


def _fill_rows():
    """40 host-frame calls on one slot: every call's previous rectangle is the one the call before it wrote"""
    rng = np.random.default_rng(77)
    W, H = FILL_W, FILL_H
    out, prev = [], None
    for i in range(40):
        x0, x1 = sorted(int(v) for v in rng.integers(0, W, 2))
        y0, y1 = sorted(int(v) for v in rng.integers(0, H, 2))
        roi, flags, bg = (x0, y0, x1, y1), HOST | DEPTH | COLS, 1.0
        if i in (0, 17):  # the slot's first call and a changed background: everything counts
            flags |= ALL_BG
        if i >= 17:
            bg = 0.25
        if i in (5, 6, 30):  # empty regions, two in a row
            roi = (0, 0, -1, -1)
        if i in (9, 21, 22):  # identical rectangles
            roi = out[-1]["rois"][0]
        if i in (12, 13, 25):  # whole rows (the copies of a progressive call)
            flags &= ~COLS
        if i == 14:  # x1 <= x0: rows of a region that lies beside the frame travel as whole rows
            roi = (W + 16, 8, W + 20, 20)
        if i == 33:
            roi = (0, 0, W - 1, H - 1)
        out.append(_row(f"fill-{i:02d}", W, H, rois=[roi], flags=flags, bg=bg, prev=(0, H, 0, W) if i == 0 else None, prev_from=prev))
        prev = out[-1]["name"]
    return out


def rows():
    out = _geometry_rows() + _region_rows() + _queue_rows() + _band_rows() + _fill_rows()
    names = [r["name"] for r in out]
    assert len(set(names)) == len(names)
    return out


class Plan:
    """nrf_debug_frame_plan's answer, by section"""

    def __init__(self, row, flat):
        n = row["n_views"]
        self.flat = flat
        self.head = dict(zip(HEAD, (int(v) for v in flat[:24])))
        p = 24
        per_view = flat[p:p + 8 * n].reshape(n, 8)
        self.roi, self.rows = per_view[:, :4], per_view[:, 4:]
        p += 8 * n
        lv = self.head["launch_views"]
        self.queues = flat[p:p + 5 * lv].reshape(lv, 5)  # k_lo, k_hi, q_begin, q_rows, q_row0
        p += 5 * lv
        self.bands = self.copies = self.fills = None
        if row["flags"] & HOST:
            nb = self.head["n_bands"]
            self.bands = flat[p:p + 5 * nb].reshape(nb, 5)  # view, lo, hi, s0, s1
            p += 5 * nb
            self.copies = flat[p:p + 9 * n].reshape(n, 9)  # pitched, rgb {off, pitch, width, rows}, depth {...}
            p += 9 * n
            self.fills = flat[p:p + 21 * n].reshape(n, 21)  # n, 4 x {r0, r1, c0, c1}, now {r0, r1, c0, c1}
            p += 21 * n
        assert p == len(flat)


def _debug_fn(lib):
    fn = lib.nrf_debug_frame_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_void_p]
    return fn


def plan(row, prev=None, lib=None):
    """nrf_debug_frame_plan of a row (prev: the fill's previous rectangle where the row takes it from another row's answer)"""
    fn = _debug_fn(lib or nh.load_library())
    prev = row["prev"] if row["prev"] is not None else prev
    ints = np.array([row["W"], row["H"], row["shard"][0], row["shard"][1], row["n_views"], row["n_cus"], row["waves"], row["classes"], row["plan_max_pos"],
                     row["plan_cap"], row["dil_bytes"], row["flags"], *prev, RENDER_WAVES], np.int32)
    fin = np.array([row["scale"], row["bg"], *row["box"]], np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    cams = None if row["cams"] is None else np.ascontiguousarray(row["cams"], np.float32).reshape(-1, 4)
    poses = None if row["poses"] is None else np.ascontiguousarray(row["poses"], np.float32).reshape(-1, 16)
    rois = None if row["rois"] is None else np.ascontiguousarray(row["rois"], np.int32).reshape(-1, 4)
    out = np.zeros(24 + 43 * row["n_views"] + 5 * 1024, np.int64)
    n = C.c_int64()
    rc = fn(ptr(ints), ptr(fin), ptr(cams), ptr(poses), ptr(rois), ptr(out), len(out), C.byref(n))
    assert rc == nh.NRF_OK, (row["name"], rc)
    return Plan(row, out[:n.value].copy())


def plan_all(all_rows, lib=None):
    """{name: Plan}; the rows of the fill sequence take their previous rectangle from the row before"""
    out = {}
    for r in all_rows:
        prev = out[r["prev_from"]].fills[0, 17:21] if r["prev_from"] else None
        out[r["name"]] = plan(r, prev, lib)
    return out


LONG = 512  # a longer answer is recorded as its head, its length and the crc32 of the rest


def entry(p):
    flat = [int(v) for v in p.flat]
    if len(flat) <= LONG:
        return flat
    return {"head": flat[:24], "n": len(flat), "crc32": zlib.crc32(np.asarray(flat[24:], np.int64).tobytes())}


def record(lib_path, out_path=GOLDEN):
    plans = plan_all(rows(), C.CDLL(str(lib_path)))
    Path(out_path).write_text(json.dumps({k: entry(p) for k, p in plans.items()}, separators=(",", ":")) + "\n")


def golden():
    return json.loads(GOLDEN.read_text())


def golden_plan(row, g):
    """the parent's answer to a row as a Plan (short answers only)"""
    return Plan(row, np.asarray(g[row["name"]], np.int64))
