"""The Python side of host/stage_plan_check.cpp: builds the program (plain g++, no library) and parses its rows -- the launch geometry of
the stage kernels and the pixel-format kernels as csrc/nrf_stage_plan.h states it and the launchers use it.  tests/test_stage_plan_cpu.py
holds the rows to the closed form; tests/test_stage_trips_gpu.py takes every "one pass" and every trip count from here, so that a changed
cap moves the tests' sizes with it."""
import shutil
import subprocess
import tempfile
from collections import namedtuple
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "nerf-cuda_amd" / "host"
SOURCES = ("host/stage_plan_check.cpp", "csrc/nrf_stage_plan.h")

# the kinds of the program (a name, ":arg" where the geometry depends on one) -> work items per row of the call
KINDS = {
    "mlp_forward:30": 1, "mlp_forward:20": 1, "mlp_forward:21": 1, "gen_mlp_forward": 1, "encode_grid": 16, "gen_encode_grid:8": 8,
    "gen_encode_grid:12": 12, "gen_encode_grid:16": 16, "encode_dir": 1, "gen_encode_dir": 1, "network": 1, "generate_rays": 1, "march": 1,
    "composite": 1, "quantize": 1, "quantize_rgbd8": 1, "untile": 1, "untile_u8": 1,
}

Row = namedtuple("Row", "kind n workgroups block items_per_wg cap items_per_row items_per_pass trips_first trips_last")

_PROGRAM = None
_KEEP = None


def compiler():
    return shutil.which("g++") or shutil.which("c++")


def program():
    """host/stage_plan_check.cpp built plainly, once per process, in a temporary directory"""
    global _PROGRAM, _KEEP
    if _PROGRAM is None:
        cxx = compiler()
        assert cxx is not None, "no host C++ compiler"
        _KEEP = tempfile.TemporaryDirectory(prefix="stage_plan_")
        exe = Path(_KEEP.name) / "stage_plan_check"
        subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", str(exe), str(HOST / "stage_plan_check.cpp")], check=True)
        _PROGRAM = exe
    return _PROGRAM


def rows(pairs, exe=None):
    """[(kind, n)] -> [Row], in order"""
    pairs = list(pairs)
    text = "".join(f"{k} {int(n)}\n" for k, n in pairs)
    out = subprocess.run([str(exe or program())], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = []
    for ln in out.stdout.splitlines():
        t = ln.split()
        got.append(Row(t[0], *(int(v) for v in t[1:])))
    assert [(r.kind, r.n) for r in got] == [(k, int(n)) for k, n in pairs]
    return got


def one_pass(kind):
    """the most rows one pass of the kind's capped grid consumes"""
    return rows([(kind, 1)])[0].items_per_pass


def trips(kind, n):
    """(first worker's trips, last worker's trips) of a call with n rows"""
    r = rows([(kind, n)])[0]
    return r.trips_first, r.trips_last
