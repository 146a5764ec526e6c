"""nrf_ray_hits, the parts that need no GPU: the declaration and the binding; the equivalence the GPU tests rest on, stated on the
checker (tests/ray_hits_oracle.py) -- a hit record is what the density-only call yields when it is clipped at the crossing sample's
end, and just below its start --; the conditions under which the GPU scenes say something; the host function that sizes the
per-round sample queue for a threshold; the 13 RAYS_HIT kernel symbols of the built library; the sanitizer driver of that function.
Every test here needs the new symbol (or the new function): none passes without the feature."""
import ctypes as C
import functools
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import nerfhip as nh
import ray_hits_oracle as rho
import rays_clip_oracle as rco
import rays_forms as rf
import test_render_rays_clip_cpu as ccpu

ROOT = Path(__file__).resolve().parent.parent
MODELS = ["bound1", "bound4-cascade3", "h30", "sine-h30"]
OPACITIES = [0.5, 0.9, 0.99]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scene(name):
    """desc, the oracle, the orbit camera's 64 x 48 rays, the unlimited frame (rgba, depth, samples) of tests/rays_oracle.py"""
    desc, keep, orc, o, d, full = ccpu._scene(name) if name in ccpu.SMALL else rf.scene(name)
    assert len(o) == rf.RW * rf.RH == ccpu.W * ccpu.H
    return desc, orc, o, d, full


@functools.lru_cache(maxsize=None)
def _hits(name, opacity):
    """The checker's records of a scene at a threshold, computed once and shared (read-only)"""
    desc, orc, o, d, full = _scene(name)
    h = rho.ray_hits(orc, desc, o, d, opacity)
    for a in (h.records, h.depth, h.hit, h.margin):
        a.setflags(write=False)
    return h


# ---------------------------------------------------------------- 1. the declaration
def test_the_header_declares_it_and_the_binding_has_it():
    header = (ROOT / "include" / "nerfhip.h").read_text()
    m = re.search(r"\bint\s+nrf_ray_hits\s*\(([^)]*)\)\s*;", header)
    assert m is not None
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["nrf_context* ctx", "int n_views", "const nrf_rays* rays", "float opacity", "void* stream", "nrf_frame* out"]
    assert "nrf_ray_hits" in nh.exported_symbols()
    lib = nh.load_library()
    assert lib.nrf_ray_hits.argtypes[3] is C.c_float and lib.nrf_ray_hits.restype is C.c_int
    assert callable(getattr(nh.NerfHip, "ray_hits"))
    assert nh.NRF_ABI_VERSION == 7 == lib.nrf_abi_version()  # an addition: no structure changes
    assert re.search(r"\bNRF_RAYS_DENSITY_ONLY\s*=\s*4\b", header) and not re.search(r"\bNRF_RAYS_\w+\s*=\s*(2|8)\b", header)  # no new flag bit


# ---------------------------------------------------------------- 2. the equivalence the GPU tests rest on
@pytest.mark.parametrize("opacity", OPACITIES)
@pytest.mark.parametrize("model", MODELS)
def test_a_record_is_the_density_only_ray_clipped_at_the_crossing_sample(model, opacity):
    desc, orc, o, d, full = _scene(model)
    h = _hits(model, opacity)
    hit, rec = h.hit, h.records
    p = np.float32(opacity)
    assert hit.any() and (~hit).any()
    inf = np.float32(np.inf)
    # (A) t_max = the crossing sample's composited t: the ray ends WITH that sample
    A = rco.render(orc, desc, o, d, t_max=np.where(hit, rec[:, 0], inf).astype(np.float32))
    assert np.array_equal(_bits(A[0][:, 3]), _bits(rec[:, 3])), "weight sums, clipped at the crossing sample's end"
    assert np.array_equal(_bits(A[3]), _bits(h.depth)), "raw depth"
    assert A[2] == h.n_composited
    # (B) t_max just below the crossing sample's start: the ray ends BEFORE it
    B = rco.render(orc, desc, o, d, t_max=np.where(hit, rho.lowered(rec), inf).astype(np.float32))
    assert np.array_equal(_bits(B[0][hit, 3]), _bits(rec[hit, 2])), "weight sums, clipped below the crossing sample's start"
    assert np.all(rec[hit, 2] < p) and np.all(rec[hit, 3] >= p)
    # misses: the unlimited frame's alpha bits, nothing else in the record
    assert np.array_equal(_bits(rec[~hit, 3]), _bits(full[0][~hit, 3])) and np.all(rec[~hit, 3] < p)
    assert np.all(rec[~hit, :3] == 0)
    assert np.all(rec[hit, 1] >= np.float32(0.0034)) and np.all(rec[hit, 0] > rec[hit, 1])


# ---------------------------------------------------------------- 3. the GPU scenes say something
def test_the_scenes_have_hits_misses_and_fewer_samples():
    for model in ("bound1", "bound4-cascade3", "h30"):
        h = _hits(model, 0.5)
        share = float(np.mean(h.hit))
        touched = float(np.mean(h.records[:, 3] > 0))
        grazed = float(np.mean(~h.hit & (h.records[:, 3] > 0)))
        print(f"{model} at 0.5: hit share {share:.3f}, alpha > 0 on {touched:.3f}, misses with alpha > 0 {grazed:.3f}")
        assert share >= 0.4
        assert grazed >= 0.005
    print(f"sine-h30 at 0.5: hit share {float(np.mean(_hits('sine-h30', 0.5).hit)):.3f}")
    assert float(np.mean(_hits("sine-h30", 0.5).hit)) >= 0.1
    full = _scene("bound1")[4]
    counts = [_hits("bound1", p).n_composited for p in OPACITIES]
    print(f"bound1: composited {counts} at {OPACITIES}, {full[2]} without a threshold")
    assert 0 < counts[0] < counts[1] < counts[2] < full[2]


def test_the_uncertain_share_at_one_half_is_small():
    """What keeps GPU test 5 honest: a ray is `certain` when no sample of it brought the weight sum within 2 / 255 (the project's
    frame tolerance) of the threshold; at 0.5 at most 0.12 of the checker's hit rays are not."""
    for model in ("bound1", "bound4-cascade3", "h30"):
        h = _hits(model, 0.5)
        uncertain = float(np.mean(h.margin[h.hit] < np.float32(2.0 / 255.0)))
        print(f"{model}: uncertain share of the hit rays at 0.5: {uncertain:.3f}")
        assert uncertain <= 0.12


# ---------------------------------------------------------------- 4. the exponent of the sample queue
def _cap_exponent(opacity):
    lib = nh.load_library()
    fn = lib.nrf_debug_hit_cap_exponent
    fn.restype, fn.argtypes = C.c_int, [C.c_float]
    return int(fn(np.float32(opacity)))


def test_the_cap_exponent_table():
    """clamp(exponent(T) - e, 1, 8) samples per round: e is the binary (frexp) exponent of fp32(1 - opacity)"""
    assert _cap_exponent(0.5) == 0        # 0.5  = 0.5  * 2^0: a ray at T = 1 (exponent 1) queues one sample
    assert _cap_exponent(0.9) == -3       # 0.1  = 0.8  * 2^-3: four
    assert _cap_exponent(0.99) == -6      # 0.01 = 0.64 * 2^-6: seven
    assert _cap_exponent(np.nextafter(np.float32(1), np.float32(0))) == -13  # 2^-24 lies below T < 1e-4: today's rule bounds it
    assert _cap_exponent(1.0) == -13      # today's rule: T < 1e-4 = 0.82 * 2^-13
    for p in (0.25, 0.5, 0.75, 0.9, 0.99, 0.999, 0.9999):
        e = np.frexp(np.float32(1) - np.float32(p))[1]
        assert _cap_exponent(p) == max(int(e), -13), p
    assert [_cap_exponent(p) for p in (0.0, -0.5, 1.5, float("nan"))] == [-13] * 4  # (what the entry point refuses: nothing raised)


# ---------------------------------------------------------------- 5. the instances
def _kernel_names(tmp_path):
    """demangled names of the kernels in the gfx950 code objects inside libnerfhip.so, from their symbol tables"""
    llvm = Path("/opt/rocm/lib/llvm/bin")
    if not (llvm / "clang-offload-bundler").exists() or shutil.which("objcopy") is None:
        pytest.skip("ROCm LLVM tools not available")
    lib = ROOT / "nerf-cuda_amd" / "libnerfhip.so"
    fat = tmp_path / "fat.bin"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(lib), str(fat)], check=True)
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
    syms = set()
    for i, a in enumerate(starts):
        part, co = tmp_path / f"fat{i}.bin", tmp_path / f"dev{i}.co"
        part.write_bytes(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.run([str(llvm / "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={part}", f"--output={co}"], check=True)
        if not co.stat().st_size:
            continue
        for ln in subprocess.run([str(llvm / "llvm-objdump"), "-t", str(co)], check=True, capture_output=True, text=True).stdout.splitlines():
            f = ln.split()
            if ".text" in f and "F" in f[1:f.index(".text")]:
                syms.add(f[-1])
    syms = sorted(syms)
    names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.splitlines()
    return [n.split("(")[0] for n in names]


def test_the_library_holds_thirteen_hit_instances(tmp_path):
    by_mode = {}
    for name in _kernel_names(tmp_path):
        m = re.search(r"\b(render_kernel|render_persistent_kernel)<([^>]*)>", name)
        if not m:
            continue
        args = [a.strip() for a in m.group(2).split(",")]
        at = 4 if m.group(1) == "render_kernel" else 5  # the RAYS argument: 0 pinhole, 1 rays, 2 density-only rays, 3 ray hits
        by_mode.setdefault(args[at], []).append((m.group(1), args, at))
    hit = by_mode.get("3", [])
    assert len(hit) == 13, [(k, a) for k, a, _ in hit]
    assert sum(k == "render_persistent_kernel" for k, _, _ in hit) == 3 and sum(k == "render_kernel" for k, _, _ in hit) == 10
    dens = {(k, tuple(a)) for k, a, _ in by_mode.get("2", [])}
    assert len(dens) == 13
    for k, args, at in hit:  # each is the twin of a density-only instance, FAST stays last and off
        assert (k, tuple(args[:at] + ["2"] + args[at + 1:])) in dens, (k, args)
        assert k == "render_kernel" or args[-1] == "false"
    assert set(by_mode) == {"0", "1", "2", "3"}


# ---------------------------------------------------------------- 6. the sanitizer driver
def test_the_sanitizer_driver_of_the_cap_exponent(tmp_path):
    """host/hit_cap_asan.cpp (make -C nerf-cuda_amd/host hit_asan): a stand-alone program, AddressSanitizer + UBSan, no GPU, no library"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    host = ROOT / "nerf-cuda_amd" / "host"
    exe = tmp_path / "hit_cap_asan"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", str(exe), str(host / "hit_cap_asan.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-400:], out.stderr[-400:])
    assert out.returncode == 0 and re.search(r"hit_cap_asan: \d+ runs, 0 failed", out.stdout)
    mk = (host / "Makefile").read_text()
    assert re.search(r"^hit_asan: hit_cap_asan$", mk, re.M) and "-fsanitize=address,undefined" in mk.split("hit_cap_asan: hit_cap_asan.cpp")[1].split("\n# ")[0]
