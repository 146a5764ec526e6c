"""nrf_rb_enable_upscale / nrf_rb_upscale and the calls around them, the parts that need no GPU: the declarations and the bindings, the
upscale kernel's symbols in the built library, the one text of the definition -- host/upscale_plan_check.cpp (csrc/nrf_upscale_plan.h,
plain and under AddressSanitizer + UBSan through `make upscale_asan`) against tests/upscale_replay.py, the numpy replay the GPU tests use,
bit for bit --, the exact consequences of the definition, and what the filter is for: it beats bilinear interpolation on an analytic
image by at least 2 dB.  Every test here needs the feature: none passes without it."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import nerfhip as nh
import test_ray_hits_cpu as hcpu
import upscale_replay as ur

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "nerf-cuda_amd" / "host"
F = np.float32
AMOUNTS = (0.0, 0.5, 2.0)


# ---------------------------------------------------------------- 1. the declarations
def test_the_header_declares_them_and_the_binding_has_them():
    header = (ROOT / "include" / "nerfhip.h").read_text()
    want = {
        "nrf_rb_enable_upscale": ["nrf_render_buffer* rb", "int out_width", "int out_height"],
        "nrf_rb_disable_upscale": ["nrf_render_buffer* rb"],
        "nrf_rb_set_upscale_sharpening": ["nrf_render_buffer* rb", "float amount"],
        "nrf_rb_resolutions": ["nrf_render_buffer* rb", "int in_wh[2]", "int out_wh[2]"],
        "nrf_rb_upscale": ["nrf_render_buffer* rb", "void* rgba8", "void* stream"],
        "nrf_rb_upscaled": ["nrf_render_buffer* rb", "void** plane"],
        "nrf_rb_read_upscaled": ["nrf_render_buffer* rb", "float* rgba"],
    }
    lib = nh.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(nh.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(nrf_[a-z0-9_]+)\b", out))
    for name, args in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m is not None, name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == args, name
        assert name in nh.exported_symbols() and name in exported
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(args), name
    assert lib.nrf_rb_set_upscale_sharpening.argtypes[1] is C.c_float
    assert "(csrc/nrf_upscale_plan.h is this text as code.)" in header
    assert nh.NRF_ABI_VERSION == 7 == lib.nrf_abi_version()  # additions: no structure changes
    for method in ("enable_upscale", "disable_upscale", "set_upscale_sharpening", "resolutions", "upscale", "upscaled_ptr", "read_upscaled"):
        assert callable(getattr(nh.RenderBuffer, method)), method
    mirror = (HOST / "render_buffer.h").read_text()
    for method in ("enable_upscale", "disable_upscale", "set_upscale_sharpening", "in_resolution", "out_resolution", "upscale", "upscaled_host"):
        assert re.search(r"\b" + method + r"\s*\(", mirror), method
    testbed = (HOST / "testbed.cpp").read_text()
    assert '"--upscale"' in testbed and '"--upscale_sharpening"' in testbed and "upscaled.png" in testbed


def test_the_library_holds_the_upscale_kernel(tmp_path):
    names = hcpu._kernel_names(tmp_path)
    found = sorted(m.group(1) for m in (re.search(r"\bupscale_kernel<(\w+)>", n) for n in names) if m)
    assert found == ["false", "true"], found  # without and with the packed 8-bit plane


# ---------------------------------------------------------------- 2. one text of the definition
def _plane(seed, w, h):
    """random finite texels, some negative and some above 1"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 1.5, (h, w, 4)).astype(np.float32)
    p[rng.random((h, w, 4)) < 0.1] *= F(3.0)
    p[0, 0, :2] = F([-0.25, 1.75])  # (also where the plane is one texel)
    return p


def _run(exe, plane, ow, oh, amount):
    ih, iw = plane.shape[:2]
    text = f"{iw} {ih} {ow} {oh} {int(ur.bits(F(amount)).reshape(-1)[0]):08x}\n"
    text += "\n".join(" ".join(f"{w:08x}" for w in t) for t in ur.bits(plane).reshape(-1, 4)) + "\n"
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln.split() for ln in out.stdout.splitlines()]
    assert lines[0][0] == "plan"
    if lines[0][1] == "0":
        return None
    words = np.array([[int(w, 16) for w in ln] for ln in lines[1:]], np.uint32).reshape(oh, ow, 5)
    return [int(w, 16) for w in lines[0][2:]], words


# (source, target): ratio 2; two non-integer ratios; identity; ratio 4, where the clamped border taps dominate; every clamp at once;
# ratio 8 on one axis and 1 on the other
CASES = [((5, 3), (10, 6)), ((7, 5), (9, 8)), ((4, 4), (4, 4)), ((3, 2), (12, 8)), ((1, 1), (3, 3)), ((2, 16), (16, 16))]


def test_the_plan_header_and_the_numpy_replay_are_one_definition(tmp_path):
    """host/upscale_plan_check.cpp, a stand-alone program (no GPU, no library): a plane in, every output texel's bits and packed dword
    out, held to tests/upscale_replay.py bit for bit -- built plainly, and once more through `make upscale_asan` (AddressSanitizer +
    UBSan) in a copy of the two directories the rule needs."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    plain = tmp_path / "upscale_plan_check"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-o", str(plain), str(HOST / "upscale_plan_check.cpp")], check=True)
    work = tmp_path / "tree" / "nerf-cuda_amd"
    (work / "host").mkdir(parents=True)
    (work / "csrc").mkdir()
    for rel in ("host/Makefile", "host/upscale_plan_check.cpp", "csrc/nrf_upscale_plan.h"):
        shutil.copy(ROOT / "nerf-cuda_amd" / rel, work / rel)
    r = subprocess.run(["make", "-C", str(work / "host"), "upscale_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "-fsanitize=address,undefined" in r.stdout and "-ffp-contract=off" in r.stdout and "2 x 2 -> 3 x 4, 12 texels" in r.stderr + r.stdout
    assert re.search(r"^upscale_asan: upscale_plan_check$", (HOST / "Makefile").read_text(), re.M)
    for exe in (plain, work / "host" / "upscale_plan_check"):
        for k, ((iw, ih), (ow, oh)) in enumerate(CASES):
            plane = _plane(300 + k, iw, ih)
            assert (plane < 0).any() and (plane > 1).any()
            for amount in AMOUNTS:
                (rx, ry), words = _run(exe, plane, ow, oh, amount)
                assert [rx, ry] == [int(ur.bits(F(iw) / F(ow)).reshape(-1)[0]), int(ur.bits(F(ih) / F(oh)).reshape(-1)[0])]
                want, packed = ur.upscale(plane, ow, oh, amount)
                bad = np.nonzero(np.any(words[:, :, :4] != ur.bits(want), axis=2))
                assert len(bad[0]) == 0, ((iw, ih), (ow, oh), amount, len(bad[0]), bad[0][:5], bad[1][:5])
                assert np.array_equal(words[:, :, 4], packed), ((iw, ih), (ow, oh), amount)
        # refused plans: below the source, beyond 8 x, beyond 16384, a bad amount
        one = _plane(1, 1, 1)
        for (ow, oh), amount in [((0, 1), 0.0), ((9, 1), 0.0), ((1, 9), 0.0), ((8, 8), 2.5), ((8, 8), -0.1), ((8, 8), np.nan)]:
            assert _run(exe, one, ow, oh, amount) is None, (ow, oh, amount)
        assert _run(exe, _plane(2, 3, 1), 2, 1, 0.0) is None and not ur.axis_valid(3, 2) and not ur.axis_valid(2049, 16385)


# ---------------------------------------------------------------- 3. the exact consequences of the definition
def test_equal_resolutions_and_amount_zero_return_the_surface():
    for seed, (w, h) in enumerate([(4, 4), (33, 17), (1, 1), (2, 9)]):
        plane = _plane(400 + seed, w, h)
        out, _ = ur.upscale(plane, w, h, 0.0)
        assert np.array_equal(out, plane)  # as values (w1 = 1 and the other weights are zeros at t = 0)


def test_amount_zero_makes_the_second_stage_the_identity_bit_for_bit():
    for k, ((iw, ih), (ow, oh)) in enumerate(CASES + [((19, 11), (38, 22)), ((23, 9), (37, 17))]):
        U = ur.reconstruct(_plane(500 + k, iw, ih), ow, oh)
        assert np.array_equal(ur.bits(ur.sharpen(U, 0.0)), ur.bits(U))


def test_a_constant_plane_stays_constant_bit_for_bit():
    texel = F([0.3, -1.7, 2.5, 1e-3])
    for (iw, ih), (ow, oh) in CASES + [((16, 9), (31, 70)), ((5, 5), (40, 40))]:
        plane = np.broadcast_to(texel, (ih, iw, 4)).copy()
        for amount in AMOUNTS:
            out, packed = ur.upscale(plane, ow, oh, amount)
            assert np.array_equal(ur.bits(out), np.broadcast_to(ur.bits(texel), (oh, ow, 4))), ((iw, ih), (ow, oh), amount)
            assert np.all(packed == ur.rgba8(texel))


def test_a_single_texel_upscales_to_copies_of_itself():
    texel = _plane(7, 1, 1)
    for ow, oh in [(1, 1), (3, 3), (4, 4), (8, 5)]:
        for amount in AMOUNTS:
            out, _ = ur.upscale(texel, ow, oh, amount)
            assert np.array_equal(ur.bits(out), np.broadcast_to(ur.bits(texel), (oh, ow, 4)))


def test_every_output_channel_lies_within_the_sources_range():
    for k, ((iw, ih), (ow, oh)) in enumerate(CASES + [((19, 11), (38, 22)), ((23, 9), (37, 17)), ((13, 7), (52, 28))]):
        plane = _plane(600 + k, iw, ih)
        for amount in AMOUNTS:
            out, _ = ur.upscale(plane, ow, oh, amount)
            assert np.all(out >= plane.min(axis=(0, 1))) and np.all(out <= plane.max(axis=(0, 1)))


def test_the_fractions_and_the_indices_stay_in_range_up_to_the_limits():
    sizes = [(1, 1), (1, 8), (2, 16), (3, 7), (540, 1080), (1080, 1920), (2048, 16384), (2049, 16384), (16383, 16384), (16384, 16384),
             (5461, 16383), (4099, 16381), (12289, 16384)]
    rng = np.random.default_rng(11)
    for _ in range(200):
        n_in = int(rng.integers(1, 16385))
        sizes.append((n_in, int(rng.integers(n_in, min(8 * n_in, 16384) + 1))))
    for n_in, n_out in sizes:
        assert ur.axis_valid(n_in, n_out)
        i, f, taps = ur.geometry(n_in, n_out)
        assert f.dtype == np.float32 and np.all(f >= 0) and np.all(f < 1), (n_in, n_out)
        assert i.min() >= -1 and i.max() <= n_in - 1, (n_in, n_out, i.min(), i.max())
        assert np.all(np.diff(i) >= 0)                               # monotonic: a tile's footprint runs from its first tap to its last
        assert taps.min() >= 0 and taps.max() <= n_in - 1


# ---------------------------------------------------------------- 4. what the filter is for
def _analytic(w, h):
    """four channels sampled at the pixel centres of the unit square"""
    x = ((np.arange(w) + 0.5) / w)[None, :]
    y = ((np.arange(h) + 0.5) / h)[:, None]
    wave = 0.5 + 0.5 * np.sin(9 * x + 4 * y) * np.cos(7 * y - 2 * x)
    edge = 1.0 / (1.0 + np.exp(-40.0 * (0.8 * x + 0.6 * y - 0.7)))
    ring = np.exp(-0.5 * ((np.hypot(x - 0.5, y - 0.45) - 0.3) / 0.04) ** 2)
    disc = 1.0 / (1.0 + np.exp(60.0 * (np.hypot(x - 0.5, y - 0.5) - 0.4)))
    return np.stack([wave, edge, ring, disc], axis=2)


def _psnr(a, b):
    return 10.0 * np.log10(1.0 / np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))


@pytest.mark.parametrize("src,dst", [((48, 32), (96, 64)), ((48, 32), (72, 48)), ((40, 30), (53, 41)), ((24, 16), (96, 64))])
def test_the_reconstruction_beats_bilinear_by_two_decibels(src, dst):
    low, high = _analytic(*src).astype(np.float32), _analytic(*dst)
    base = _psnr(ur.bilinear64(low, *dst), high)
    for amount in (0.0, 0.25):
        got = _psnr(ur.upscale(low, dst[0], dst[1], amount)[0], high)
        print(f"{src} -> {dst} at amount {amount}: {got:.2f} dB against bilinear's {base:.2f} dB (+{got - base:.2f})")
        assert got >= base + 2.0, (src, dst, amount, got, base)
