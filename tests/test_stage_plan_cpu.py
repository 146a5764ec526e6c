"""csrc/nrf_stage_plan.h, the launch geometry of the stage kernels and the pixel-format kernels, without a GPU: host/stage_plan_check.cpp
(built plainly, and under AddressSanitizer + UBSan through `make stage_asan`) against the closed form
    workgroups = min(cap, max(1, ceil(n * items_per_row / items_per_wg)))
for every kind at 0, 1, either side of a workgroup's and of a pass's edge and 2^32 - 1 rows, and against TODAY, the figures the
kernels have as this is written.  tests/test_stage_trips_gpu.py sizes its calls from the program's output, so a changed cap moves those
sizes with it; the one line of TODAY that then fails here says which kernel's pass changed."""
import re
import shutil
import subprocess

import pytest

import stage_plan_rows as spr

# kind -> (block, items per workgroup and trip, workgroup cap, rows of one pass): today's values.
# A pass of the capped grid: mlp_forward 256 * OCC workgroups x 4 waves x 32 rows (OCC 3 for form 30, 2 for forms 20 and 21);
# gen_mlp_forward and network 1024 workgroups x 4 waves x 32 / 64 rows; the grid encodings 2048 workgroups x 256 lanes, a lane per
# (sample, level); every other kernel 2048 x 256 lanes, a lane per row (untile_u8: a row is a quad of pixels when W % 4 == 0).
TODAY = {
    "mlp_forward:30": (256, 128, 768, 98304),
    "mlp_forward:20": (256, 128, 512, 65536),
    "mlp_forward:21": (256, 128, 512, 65536),
    "gen_mlp_forward": (256, 128, 1024, 131072),
    "network": (256, 256, 1024, 262144),
    "encode_grid": (256, 256, 2048, 32768),
    "gen_encode_grid:8": (256, 256, 2048, 65536),
    "gen_encode_grid:12": (256, 256, 2048, 43690),
    "gen_encode_grid:16": (256, 256, 2048, 32768),
    "encode_dir": (256, 256, 2048, 524288),
    "gen_encode_dir": (256, 256, 2048, 524288),
    "generate_rays": (256, 256, 2048, 524288),
    "march": (256, 256, 2048, 524288),
    "composite": (256, 256, 2048, 524288),
    "quantize": (256, 256, 2048, 524288),
    "quantize_rgbd8": (256, 256, 2048, 524288),
    "untile": (256, 256, 2048, 524288),
    "untile_u8": (256, 256, 2048, 524288),
}
# items one worker consumes per trip: a wave's chunk of rows in the MLP and network kernels, else one lane's item
WORKER_ITEMS = {"mlp_forward:30": 32, "mlp_forward:20": 32, "mlp_forward:21": 32, "gen_mlp_forward": 32, "network": 64}


def _ceil(a, b):
    return -(-a // b)


def _sizes(kind):
    _, wg_items, cap, pass_rows = TODAY[kind]
    per_row = spr.KINDS[kind]
    wg_lo, wg_hi = wg_items // per_row, _ceil(wg_items, per_row)  # the rows that fill a workgroup's trip, either way rounded
    edges = {wg_lo, wg_hi, pass_rows, 2 * pass_rows, _ceil(cap * wg_items, per_row)}
    out = {0, 1, 2 ** 32 - 1}
    for e in edges:
        out |= {e - 1, e, e + 1}
    return sorted(v for v in out if v >= 0)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """host/stage_plan_check.cpp built plainly, and once more through `make stage_asan` in a copy of the two directories the rule needs"""
    if spr.compiler() is None:
        pytest.skip("no host C++ compiler")
    plain = spr.program()
    work = tmp_path_factory.mktemp("stage") / "tree" / "nerf-cuda_amd"
    (work / "host").mkdir(parents=True)
    (work / "csrc").mkdir()
    for rel in ("host/Makefile",) + spr.SOURCES:
        shutil.copy(spr.ROOT / "nerf-cuda_amd" / rel, work / rel)
    r = subprocess.run(["make", "-C", str(work / "host"), "stage_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "-fsanitize=address,undefined" in r.stdout and "stage_plan_check: 8 rows" in r.stderr + r.stdout
    return plain, work / "host" / "stage_plan_check"


def test_the_kinds_are_the_same_everywhere():
    assert set(TODAY) == set(spr.KINDS)
    assert re.search(r"^stage_asan: stage_plan_check$", (spr.HOST / "Makefile").read_text(), re.M)


@pytest.mark.parametrize("kind", list(TODAY))
def test_rows_follow_the_closed_form_and_todays_values(programs, kind):
    block, wg_items, cap, pass_rows = TODAY[kind]
    per_row = spr.KINDS[kind]
    sizes = _sizes(kind)
    for exe in programs:
        got = spr.rows([(kind, n) for n in sizes], exe)
        for n, r in zip(sizes, got):
            assert (r.block, r.items_per_wg, r.cap, r.items_per_row, r.items_per_pass) == (block, wg_items, cap, per_row, pass_rows), (kind, n, r)
            assert r.workgroups == min(cap, max(1, _ceil(n * per_row, wg_items))), (kind, n, r)
            worker = WORKER_ITEMS.get(kind, 1)
            units, workers = _ceil(n * per_row, worker), r.workgroups * (wg_items // worker)
            assert (r.trips_first, r.trips_last) == (_ceil(units, workers), units // workers), (kind, n, r)
    # what "one pass" means: that many rows are one trip for every worker that has any, one row more is a second trip for the first
    at, over = spr.rows([(kind, pass_rows), (kind, pass_rows + 1)], programs[0])
    assert at.trips_first == 1 and over.trips_first == 2 and over.trips_last == 1
    assert at.workgroups == cap or per_row * pass_rows + per_row > cap * wg_items


def test_the_program_refuses_what_it_does_not_know(programs):
    for text in ("mlp_forward 1\n", "mlp_forward:31 1\n", "encode_grid:16 1\n", "gen_encode_grid 1\n", "gen_encode_grid:0 1\n", "nothing 1\n",
                 "march 18446744073709551615\n"):
        for exe in programs:
            r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
            assert r.returncode == 2 and r.stdout == "", (text, r.returncode, r.stdout)


def test_the_launchers_take_their_grids_from_the_plan():
    """every launch of a kernel of the plan names stage_grid; grid_for stays with the density grid's two kernels"""
    text = (spr.ROOT / "nerf-cuda_amd" / "csrc" / "nrf_kernels.hip").read_text()
    launches = re.findall(r"hipLaunchKernelGGL\(\(?(\w+)[^;]*?dim3\((\w+)\(", text)
    planned = {"encode_grid_kernel", "gen_encode_grid_kernel", "encode_dir_kernel", "gen_encode_dir_kernel", "mlp_forward_kernel",
               "gen_mlp_forward_kernel", "network_kernel", "generate_rays_kernel", "march_kernel", "composite_kernel", "untile_kernel",
               "quantize_kernel", "quantize_rgbd8_kernel", "untile_rgbd8_u8_kernel"}
    seen = {k for k, _ in launches}
    assert planned <= seen, planned - seen
    for kernel, fn in launches:
        if kernel in planned:
            assert fn == "stage_grid", (kernel, fn)
    assert {k for k, fn in launches if fn == "grid_for"} == {"density_positions_kernel", "density_update_kernel"}
