"""The grid side of the host's plan without a GPU (nrf_debug_grid_plan, an undeclared diagnostic of libnerfhip.so: plan_model, then
plan_grid of csrc/nrf_grid_plan.h): the march tables a density grid becomes, which of them are staged in LDS, and the workgroup that
renders the frames beside them.  The tables are checked against short numpy statements; occ_box, the visibility walk where a loaded
context shows it, and every field of the fit are pinned to what the commit before plan_grid had in its loaded context
(tests/golden/grid_plan_parent.json, tests/grid_plan_rows.py): a change of any of them is a change of behaviour."""
import zlib

import numpy as np
import pytest

import grid_plan_rows as R

HOT, GENERIC, WIDE, W16, W32, W128, WIDE_SH, DEPTH, GRID2, GRID4, GRID8, GRID1, ACT = range(13)  # (csrc/nrf_launch.h)
f32 = np.float32


def _mip_bound(cascade, level, bound):
    return min(2.0 ** min(level, 1023) if cascade > 1 else 1.0, float(f32(bound)))


def _bits(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def _reachable(H, cascade, bound):
    """[C, H, H, H]: cells of cascade k >= 1 that do not lie, with a cell of slack, inside the inner cube max|p| < 2^(k-1)"""
    out = np.ones((cascade, H, H, H), bool)
    for k in range(1, cascade):
        mb = _mip_bound(cascade, k, bound)
        cell = 2.0 * mb / H
        lo = -mb + np.arange(H) * cell
        r = np.maximum(np.abs(lo), np.abs(lo + cell))
        r_max = np.maximum(np.maximum(r[:, None, None], r[None, :, None]), r[None, None, :])
        out[k] = ~(r_max + cell < 2.0 ** min(k - 1, 1023))
    return out


@pytest.fixture(scope="module")
def golden():
    return R.golden()


@pytest.mark.parametrize("name", sorted(R.ROWS))
def test_row(name, golden):
    row = R.ROWS[name]
    H, Cs, bound = row["H"], row["cascade"], row["bound"]
    desc, keep, grid = R.build(row)
    got, box, (occ, coarse, ctab, dilated) = R.plan(desc, None, row["mean"], row["flags"])
    want = golden[name]
    cells = Cs * H ** 3

    # the tables: independent statements
    occupied = grid > np.minimum(f32(0.01), f32(row["mean"]))
    assert occ.size == (cells + 31) // 32 + 1 and np.array_equal(_bits(occ, occ.size * 32), np.pad(occupied, (0, occ.size * 32 - cells)))
    has_coarse = H % 4 == 0 and H >= 8
    assert got["coarse_shift"] == (2 if has_coarse else 0)
    Hc = H // 4
    if has_coarse:
        blocks = occupied.reshape(Cs, Hc, 4, Hc, 4, Hc, 4).any(axis=(2, 4, 6)).reshape(-1)
        assert coarse.size == (blocks.size + 31) // 32 + 1
        assert np.array_equal(_bits(coarse, coarse.size * 32), np.pad(blocks, (0, coarse.size * 32 - blocks.size)))
    else:
        assert coarse.size == 0
    v = np.arange(H + 1, dtype=f32)
    want_ctab = np.concatenate([((v / f32(H - 1)) * f32(2) - f32(1)) * f32(_mip_bound(Cs, k, bound)) for k in range(Cs)])
    assert ctab.dtype == f32 and np.array_equal(ctab.view(np.uint32), want_ctab.view(np.uint32))
    live = occupied.reshape(Cs, H, H, H) & _reachable(H, Cs, bound)
    # the visibility walk is off when positions outside the outermost cube exist and a live cell lies in a boundary layer
    aabb = row["aabb"] or (-bound,) * 3 + (bound,) * 3
    exterior = bound > _mip_bound(Cs, Cs - 1, bound) or any(a < -bound for a in aabb[:3]) or any(a > bound for a in aabb[3:])
    edge = live[:, [0, -1]].any() or live[:, :, [0, -1]].any() or live[:, :, :, [0, -1]].any()
    assert got["visibility_walk"] == int(not (exterior and edge))
    if has_coarse and got["visibility_walk"]:
        p = np.pad(live, ((0, 0), (1, 1), (1, 1), (1, 1)))
        dil = np.zeros_like(live)
        for dx in range(3):
            for dy in range(3):
                for dz in range(3):
                    dil |= p[:, dx:dx + H, dy:dy + H, dz:dz + H]
        sets = dil.reshape(Cs, Hc, 4, Hc, 4, Hc, 4).any(axis=(2, 4, 6)).reshape(Cs, -1)
        words = (Hc ** 3 + 31) // 32
        assert got["dilated_level_words"] == words and dilated.size == words * Cs
        assert np.array_equal(_bits(dilated, dilated.size * 32).reshape(Cs, -1), np.pad(sets, ((0, 0), (0, words * 32 - Hc ** 3))))
    else:
        assert dilated.size == 0 and got["dilated_level_words"] == 0

    # ... and everything against the recorded parent: fields, occ_box bit for bit, the tables as the device held them
    assert [got[k] for k in R.FIELDS] == want["fields"], dict(zip(R.FIELDS, want["fields"]))
    assert [int(b) for b in box.view(np.uint32)] == want["box_bits"]
    assert [zlib.crc32(np.ascontiguousarray(t).tobytes()) for t in (occ, coarse, ctab, dilated)] == want["crc32"]
    if has_coarse:  # (a loaded context shows the walk as the presence of the dilated table)
        assert got["visibility_walk"] == int(want["fields"][R.FIELDS.index("n_dilated")] > 0)
    # the LDS total the plan reports is what launch_render asks for: field 12 is render_persistent_launch_lds_bytes of a DevModel
    # the plan was applied to, the last value is GridFit::persistent_lds_bytes (both made by persistent_lds_total)
    assert got["persistent_lds_bytes"] == got["fit_persistent_lds_bytes"]


def _fields(golden, name):
    return dict(zip(R.FIELDS, golden[name]["fields"]))


def test_what_the_rows_are_there_for(golden):
    """Each branch the rows were chosen for is taken by the row chosen for it (in the RECORDED values: a row that stopped taking
    its branch would pin nothing)."""
    g = lambda n: _fields(golden, n)
    box = lambda n: [float(x) for x in np.array(golden[n]["box_bits"], np.uint32).view(f32)]
    for n in ("h4", "h30", "zero-h30"):  # no coarse level: no LDS tables, no dilated set, no persistent form
        assert (g(n)["coarse_shift"], g(n)["lds_coarse_words"], g(n)["n_coarse"], g(n)["n_dilated"], g(n)["persistent"]) == (0, 0, 0, 0, 0)
    assert g("h8")["n_coarse"] == 2 and g("h8")["persistent"] == 1  # Hc = 2: 8 bits + the padding word
    for n in ("zero", "zero-h30", "inner-c3"):  # nothing occupied -- or nothing a sample can reach: the empty box
        assert box(n) == [1.0, 1.0, 1.0, -1.0, -1.0, -1.0]
    assert golden["inner-c3"]["crc32"][3] == zlib.crc32(bytes(4 * 48))  # ... and no dilated bit
    assert box("inner-and-random-c3") == box("h32-pow2") and golden["inner-and-random-c3"]["crc32"][3] == golden["h32-pow2"]["crc32"][3]
    assert golden["inner-and-random-c3"]["crc32"][0] != golden["h32-pow2"]["crc32"][0]
    cell = 2.0 / 32
    assert box("cell0")[0] == -1.0 - 2 * cell and box("cell0")[3] == -1.0 + 3 * cell      # extended to the aabb (= -bound) - 2 cells
    assert box("cellH1")[4] == 1.0 + 2 * cell and box("cellH1")[1] == -1.0 + 29 * cell
    assert box("full") == [-1.0 - 2 * cell] * 3 + [1.0 + 2 * cell] * 3
    assert golden["mean-below"]["crc32"][0] != golden["mean-above"]["crc32"][0] == golden["h32-unit"]["crc32"][0]
    # exterior positions: the walk is off with an occupied boundary cell, on without; the box reaches the aabb on that side
    assert g("exterior-b4-c2-boundary")["n_dilated"] == 0 and g("exterior-b4-c2-interior")["n_dilated"] == 32
    assert g("aabb-wide-boundary")["n_dilated"] == 0 and g("aabb-wide-interior")["n_dilated"] == 16
    assert box("aabb-wide-boundary")[0] == -1.5 - 2 * cell
    # the table budget: one cascade more and the tables stay in global memory, and with them the per-strip kernel
    assert R.table_bytes(8, g("under-budget")["n_ctab"] // 9) <= R.LDS_TABLE_BUDGET < R.table_bytes(8, g("over-budget")["n_ctab"] // 9)
    assert g("under-budget")["persistent"] == 1 and g("under-budget")["lds_coarse_words"] == g("under-budget")["n_coarse"]
    assert (g("over-budget")["persistent"], g("over-budget")["lds_coarse_words"], g("over-budget")["lds_ctab_floats"]) == (0, 0, 0)
    # NET_WIDE shares a CU with two more workgroups: tables of 9476 bytes fit the 48 KiB budget, not its third of the LDS
    assert R.table_bytes(8, 256) == 9476 and (g("wide-over-its-room")["lds_coarse_words"], g("wide-over-its-room")["persistent"]) == (0, 0)
    # the per-strip kernel stages the dilated table only where it fits the weight area (20 KiB); the persistent one all of it
    assert (g("under-budget")["lds_dilated_strip"], g("under-budget")["lds_dilated_persist"]) == (1328, 1328)
    assert (g("base-strip")["lds_dilated_strip"], g("base-strip")["lds_dilated_persist"]) == (16, 0)


def test_the_fit_of_each_shape(golden):
    """(net, persist_waves, gen_weights_lds) of the recorded rows: every rung of the ladder is reached by a shape of
    tests/test_instance_plan_cpu.py."""
    fit = lambda n: tuple(_fields(golden, n)[k] for k in ("net", "persistent", "persist_waves", "gen_weights_lds", "rays_persistent"))
    own = {"base": (HOT, 1, 16, 0, 1), "freq12": (WIDE, 1, 12, 0, 0), "sh8": (WIDE_SH, 1, 8, 0, 0), "w64_h2_h2": (DEPTH, 1, 16, 0, 0),
           "F4_L8": (GRID4, 1, 16, 0, 0), "w128": (W128, 1, 12, 0, 0), "act_squareplus": (ACT, 1, 12, 0, 0)}
    for n, want in own.items():
        assert fit(n) == fit(n + "-no-wlds") == want
        stage = n if n in ("base", "freq12") else None
        assert fit(n + "-strip") == ((own[stage][0] if stage else GENERIC), 0, 0, 0, 0)
    assert fit("freq12-h96") == (WIDE, 1, 8, 0, 0)  # the generic march: 8 waves
    # the generic instance: 12 waves with its weights in LDS, 12 without, 8 with, 8 without, and no persistent form at all
    assert fit("w32_h2_h3") == (GENERIC, 1, 12, 1, 0) and fit("w32_h2_h3-no-wlds") == (GENERIC, 1, 12, 0, 0)
    assert fit("w64_h2_h2-no-own") == (GENERIC, 1, 8, 1, 0) and fit("w64_h2_h2-no-own-no-wlds") == (GENERIC, 1, 8, 0, 0)
    # w128_h1_h1 and F8_L16_w128 pass the 12-wave and the 8-wave rungs (271976 and 182000 bytes without tables) without fitting either
    for n in ("w128_h1_h1", "F8_L16_w128"):
        assert fit(n) == fit(n + "-no-wlds") == fit(n + "-strip") == (GENERIC, 0, 0, 0, 0)
