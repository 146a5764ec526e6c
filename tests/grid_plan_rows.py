"""The rows of tests/test_grid_plan_cpu.py and test_grid_plan_gpu.py: a model shape, a density grid geometry, a grid built here from
a seeded generator plus hand-placed cells, and the context flags.  tests/golden/grid_plan_parent.json holds, per row, what the
commit BEFORE plan_grid existed had in its loaded context on an MI355X (read out of nrf_context: DevModel's grid fields, rays_persistent,
the LDS bytes launch_render summed, the crc32 of the four device tables): nothing plan_grid computes was ever written into it."""
import ctypes as C
import json
import zlib
from pathlib import Path

import numpy as np

import models
import nerfhip as nh

GOLDEN = Path(__file__).resolve().parent / "golden" / "grid_plan_parent.json"
# out[] of nrf_debug_grid_readout, and the first 17 of nrf_debug_grid_plan's 19 (then: visibility_walk, GridFit::persistent_lds_bytes)
FIELDS = ("net", "stage", "persistent", "persist_waves", "gen_weights_lds", "lds_coarse_words", "lds_ctab_floats", "lds_dilated_strip",
          "lds_dilated_persist", "coarse_shift", "dilated_level_words", "rays_persistent", "persistent_lds_bytes", "n_occ", "n_coarse",
          "n_ctab", "n_dilated")
ALLOW_OWN, ALLOW_PERSISTENT, ALLOW_GEN_WLDS = 1, 2, 4
ALL = ALLOW_OWN | ALLOW_PERSISTENT | ALLOW_GEN_WLDS
LDS_TABLE_BUDGET = 48 * 1024  # (csrc/nrf_render.h LDS_MARCH_TABLE_MAX)


def table_bytes(H, cascade):
    """coarse words (+ 1 padding word) + cell-boundary floats of a grid with a coarse level"""
    return 4 * ((cascade * (H // 4) ** 3 + 31) // 32 + 1 + cascade * (H + 1))


# the smallest grid whose coarse + boundary tables exceed the LDS table budget: H = 8 is the smallest side with a coarse level, its
# tables grow by 9 floats + a quarter word per cascade, and nrf_load_model puts no upper limit on the cascades
OVER_BUDGET_CASCADES = next(c for c in range(1, 4096) if table_bytes(8, c) > LDS_TABLE_BUDGET)
assert OVER_BUDGET_CASCADES == 1329 and table_bytes(8, OVER_BUDGET_CASCADES - 1) <= LDS_TABLE_BUDGET


def make_grid(H, cascade, fill, seed=0):
    rng = np.random.default_rng(4000 + seed)
    g = np.zeros((cascade, H, H, H), np.float32)
    q, a, b = H // 4, 3 * H // 8, 5 * H // 8
    if "random" in fill:  # densities on both sides of either threshold (0.01, a mean of 0.005) in a box off the boundary layer, per cascade
        for c in range(cascade):
            lo, hi = rng.integers(1, H // 2, 3), rng.integers(H // 2 + 1, H, 3)
            sl = (c, slice(lo[0], hi[0]), slice(lo[1], hi[1]), slice(lo[2], hi[2]))
            g[sl] = (rng.uniform(0.0, 0.02, g[sl].shape) * (rng.random(g[sl].shape) < 0.3)).astype(np.float32)
        g[0, H // 2, H // 2, H // 2] = 1.0
    if "full" in fill:
        g[:] = 1.0
    if "cell0" in fill:
        g[0, 0, H // 2, H // 2] = 1.0
    if "cellH1" in fill:
        g[0, H // 2, H - 1, H // 2] = 1.0
    if "inner" in fill:  # inside the inner cube max|p| < 2^(k-1) of cascades k >= 1, more than a cell from its faces
        g[1:, a:b, a:b, a:b] = 1.0
    if "blob" in fill:
        g[:, q:H - q, q:H - q, q:H - q] = 1.0
    if "boundary" in fill:  # a boundary cell of the outermost cascade
        g[cascade - 1, H - 1, H // 2, H // 2] = 1.0
    return g.reshape(-1)


def _row(name, shape="base", H=32, cascade=1, bound=1.0, fill="random", mean=0.02, aabb=None, flags=ALL):
    return dict(name=name, shape=shape, H=H, cascade=cascade, bound=bound, fill=fill, mean=mean, aabb=aabb, flags=flags)


SHAPES = {  # (tests/test_instance_plan_cpu.py SHAPES)
    "base": dict(), "freq12": dict(dir_otype="Frequency", n_frequencies=12), "sh8": dict(sh_degree=8), "w64_h2_h2": dict(density_hidden_layers=2),
    "F4_L8": dict(n_features_per_level=4, n_levels=8), "w128": dict(n_neurons=128), "act_squareplus": dict(activation="Squareplus"),
    "w128_h1_h1": dict(n_neurons=128, density_hidden_layers=1, rgb_hidden_layers=1), "F8_L16_w128": dict(n_features_per_level=8, n_neurons=128),
    "w32_h2_h3": dict(n_neurons=32, density_hidden_layers=2, rgb_hidden_layers=3),
}
ROWS = [
    _row("h8", H=8), _row("h4", H=4), _row("h30", H=30), _row("h32-unit"),
    _row("h32-pow2", cascade=3, bound=4.0), _row("h64-b1.5-c2", H=64, cascade=2, bound=1.5),
    _row("h48-b3-c3", H=48, cascade=3, bound=3.0), _row("h128-b0.75", H=128, bound=0.75),
    _row("zero", fill="zero"), _row("zero-h30", H=30, fill="zero"), _row("full", fill="full"), _row("full-c3", cascade=3, bound=4.0, fill="full"),
    _row("cell0", fill="cell0"), _row("cellH1", fill="cellH1"), _row("cell0-h8", H=8, fill="cell0"), _row("cellH1-h8", H=8, fill="cellH1"),
    _row("inner-c3", cascade=3, bound=4.0, fill="inner"), _row("inner-and-random-c3", cascade=3, bound=4.0, fill="inner random"),
    _row("mean-below", mean=0.005), _row("mean-above", mean=0.5),
    _row("exterior-b4-c2-boundary", cascade=2, bound=4.0, fill="blob boundary"), _row("exterior-b4-c2-interior", cascade=2, bound=4.0, fill="blob"),
    _row("aabb-wide-boundary", aabb=(-1.5, -1.0, -1.0, 1.0, 1.25, 1.0), fill="blob cell0"),
    _row("aabb-wide-interior", aabb=(-1.5, -1.0, -1.0, 1.0, 1.25, 1.0), fill="blob"),
    _row("over-budget", H=8, cascade=OVER_BUDGET_CASCADES), _row("under-budget", H=8, cascade=OVER_BUDGET_CASCADES - 1),
    _row("freq12-h96", shape="freq12", H=96), _row("wide-over-its-room", shape="freq12", H=8, cascade=256),
]
for _s in SHAPES:
    ROWS += [_row(_s, shape=_s), _row(_s + "-strip", shape=_s, flags=ALL & ~ALLOW_PERSISTENT),
             _row(_s + "-no-wlds", shape=_s, flags=ALL & ~ALLOW_GEN_WLDS)]
# the generic instance's ladder: w32_h2_h3 fits with 12 waves; w64_h2_h2 without its own instance (NRF_WIDTH_INSTANCES=0) only with 8
ROWS += [_row("w64_h2_h2-no-own", shape="w64_h2_h2", flags=ALL & ~ALLOW_OWN),
         _row("w64_h2_h2-no-own-no-wlds", shape="w64_h2_h2", flags=ALL & ~ALLOW_OWN & ~ALLOW_GEN_WLDS)]
ROWS = {r["name"]: r for r in ROWS}
GPU_ROWS = ("h32-unit", "h32-pow2", "h30", "h64-b1.5-c2", "freq12", "sh8", "w128_h1_h1", "base-strip")  # + GENERATED: test_grid_plan_gpu.py
GENERATED = "generated"  # golden entry of a model loaded without a grid after nrf_generate_density_grid (base shape, H = 32)


def build(row, with_grid=True):
    """(desc, keepalive, grid): the row's descriptor at log2 T = 12 carrying the row's grid (with_grid=False: none)"""
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=row["H"], cascade=1, bound=row["bound"], **SHAPES[row["shape"]])
    grid = np.ascontiguousarray(make_grid(row["H"], row["cascade"], row["fill"]))
    desc.cascade = row["cascade"]
    desc.mean_density = row["mean"]
    if row["aabb"]:
        desc.aabb = (C.c_float * 6)(*row["aabb"])
    desc.density_grid = grid.ctypes.data_as(C.POINTER(C.c_float)) if with_grid else None
    desc.n_density_grid = grid.size if with_grid else 0
    return desc, (keep, grid), grid


def env_of(flags):
    """the environment nrf_create reads those flags from"""
    return {"NRF_WIDTH_INSTANCES": str(int(bool(flags & ALLOW_OWN))), "NRF_PERSISTENT": str(int(bool(flags & ALLOW_PERSISTENT))),
            "NRF_GEN_WLDS": str(int(bool(flags & ALLOW_GEN_WLDS)))}


def _tables(call, n):
    bufs = [np.zeros(max(int(k), 1), t) for k, t in zip(n, (np.uint32, np.uint32, np.float32, np.uint32))]
    call(*[b.ctypes.data_as(C.c_void_p) for b in bufs])
    return [b[:int(k)] for b, k in zip(bufs, n)]


def plan(desc, grid, mean, flags):
    """nrf_debug_grid_plan: (fields dict incl. visibility_walk and fit_persistent_lds_bytes, box float32[6], [occ, coarse, ctab, dilated])"""
    lib = nh.load_library()
    fn = lib.nrf_debug_grid_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p] + [C.c_void_p] * 4
    out, box = np.zeros(19, np.uint32), np.zeros(6, np.float32)
    g = grid.ctypes.data_as(C.c_void_p) if grid is not None else None

    def call(*bufs):
        rc = fn(C.byref(desc), g, mean, flags, out.ctypes.data_as(C.c_void_p), box.ctypes.data_as(C.c_void_p), *bufs)
        assert rc == nh.NRF_OK, rc
    call(None, None, None, None)
    tables = _tables(call, out[13:17])
    f = dict(zip(FIELDS, (int(v) for v in out[:17])))
    f["visibility_walk"], f["fit_persistent_lds_bytes"] = int(out[17]), int(out[18])
    return f, box, tables


def readout(ctx):
    """nrf_debug_grid_readout of a loaded context: (fields dict, box float32[6], [occ, coarse, ctab, dilated] read back from the device)"""
    fn = ctx.lib.nrf_debug_grid_readout
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_void_p] * 4
    out, box = np.zeros(17, np.uint32), np.zeros(6, np.float32)

    def call(*bufs):
        rc = fn(ctx.h, out.ctypes.data_as(C.c_void_p), box.ctypes.data_as(C.c_void_p), *bufs)
        assert rc == nh.NRF_OK, rc
    call(None, None, None, None)
    tables = _tables(call, out[13:17])
    return dict(zip(FIELDS, (int(v) for v in out))), box, tables


def record(fields, box, tables):
    """a golden entry"""
    return {"fields": [fields[k] for k in FIELDS], "box_bits": [int(v) for v in box.view(np.uint32)],
            "crc32": [zlib.crc32(np.ascontiguousarray(t).tobytes()) for t in tables]}


def golden():
    return json.loads(GOLDEN.read_text())
