"""nrf_rb_overlay_image / nrf_rb_overlay_false_color / nrf_rb_error_map, the parts that need no GPU: the declarations and the bindings,
the kernels' symbols in the built library, the one text of the definition -- host/overlay_plan_check.cpp (csrc/nrf_overlay_plan.h, plain
and under AddressSanitizer + UBSan through `make overlay_asan`) against tests/overlay_replay.py, the numpy replay the GPU tests use, bit
for bit, power rows included (both sides use this machine's libm) --, the replay's pieces against the reference's own kernels compiled
for the CPU (oracle/_ref/libref_render_buffer.so), and the exact consequences of the definition.  Every test here needs the feature:
none passes without it.

"Bit for bit" lets a NaN match any NaN (overlay_replay.same): which payload an operation hands on is the machine's choice."""
import ctypes as C
import itertools
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import nerfhip as nh
import overlay_replay as orp
import test_ray_hits_cpu as hcpu

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "nerf-cuda_amd" / "host"
F = np.float32

SURFACES = [(5, 3), (19, 11)]
IMAGES = [(1, 1), (7, 5), (40, 23)]
TYPES = [nh.IMG_BYTE, nh.IMG_HALF, nh.IMG_FLOAT]
ZOOMS = [0.5, 1.0, 3.0, -1.0, 1e-30]
CENTERS = [(0.5, 0.5), (0.1, 0.9), (2.0, 2.0)]
ALPHAS = [0.0, 0.25, 1.0]
SPACES = list(itertools.product((0, 1, 2), (0, 1)))          # render space x display space (Linear, sRGB)
CURVES = [0, 1, 2, 3]
EXPOSURES = [(0.0, 0.0, 0.0), (1.0, -1.0, 2.0), (0.5, 0.0, -0.25)]
SPECIALS = F([-0.75, 1.5, -0.0, np.inf, np.nan])             # negative, above 1, -0, +inf, NaN


# ---------------------------------------------------------------- inputs
def surface_plane(seed, w, h):
    """random texels, some negative and some above 1, with the special values in the first texels when there is room"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.25, 1.25, (h, w, 4)).astype(np.float32)
    flat = p.reshape(-1, 4)
    if len(flat) >= 8:
        flat[1, 0], flat[2, 1], flat[3, 2], flat[4, 3], flat[5, 0] = SPECIALS[0], SPECIALS[1], SPECIALS[2], SPECIALS[3], SPECIALS[4]
    return p


def image_plane(seed, iw, ih, image_data_type):
    """an image of the type with its special texels: w = 0, w > 1, negative, above 1, -0, +inf, NaN; the magic texel and alpha 0 for Byte"""
    rng = np.random.default_rng(seed)
    if image_data_type == orp.IMG_BYTE:
        t = rng.integers(0, 2 ** 32, (ih, iw), dtype=np.uint64).astype(np.uint32)
        flat = t.reshape(-1)
        if len(flat) >= 4:
            flat[0], flat[1], flat[2] = orp.MAGIC_TEXEL, 0x00C08040, 0xFFFFFFFF  # magic; alpha 0; opaque white
        else:
            flat[0] = orp.MAGIC_TEXEL if seed % 2 else 0x80C08040
        return t
    p = rng.uniform(0.0, 1.0, (ih, iw, 4)).astype(np.float32)
    p[..., :3] *= p[..., 3:4]  # premultiplied
    flat = p.reshape(-1, 4)
    if len(flat) >= 8:
        flat[0, 3] = 0.0                                   # w = 0
        flat[1, 3] = 1.5                                   # w > 1
        flat[2, 0], flat[3, 1], flat[4, 2], flat[5, 0], flat[6, 1] = SPECIALS
        flat[7, 3] = np.nan
    else:
        flat[0, 3] = 0.0 if seed % 2 else 1.5
    if image_data_type == orp.IMG_HALF:
        return p.astype(np.float16).view(np.uint16)
    return p


def _hex(a):
    return " ".join(f"{int(w):08x}" for w in orp.bits(a).reshape(-1))


def image_words(image, image_data_type):
    if image_data_type == orp.IMG_BYTE:
        return " ".join(f"{int(w):08x}" for w in image.reshape(-1))
    if image_data_type == orp.IMG_HALF:
        return " ".join(f"{int(w):04x}" for w in image.reshape(-1))
    return _hex(image)


def image_case(surface, image, image_data_type, axis, rs, ds, curve, alpha, zoom, center, exposure, bg):
    H, W = surface.shape[:2]
    ih, iw = image.shape[:2]
    return (f"I {W} {H} {iw} {ih} {image_data_type} {axis} {rs} {ds} {curve} "
            + _hex(F([alpha, zoom, center[0], center[1], *exposure, *bg])) + " " + _hex(surface) + " " + image_words(image, image_data_type))


def false_color_case(surface, tw, th, axis, emap, average, brightness, viridis):
    H, W = surface.shape[:2]
    mh, mw = emap.shape
    return f"F {W} {H} {tw} {th} {mw} {mh} {axis} {int(viridis)} " + _hex(F([brightness, average])) + " " + _hex(surface) + " " + _hex(emap)


def error_case(surface, truth, mw, mh):
    H, W = surface.shape[:2]
    return f"E {W} {H} {mw} {mh} " + _hex(surface) + " " + _hex(truth)


def run(exe, cases):
    """the program's stdout as a list of token lists"""
    out = subprocess.run([str(exe)], input="\n".join(cases) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return [ln.split() for ln in out.stdout.splitlines()]


def take_pixels(lines, at, w, h):
    """(srcx, srcy, plane) of one I or F case, and the line after it"""
    rows = lines[at:at + w * h]
    assert len(rows) == w * h
    src = np.array([[int(r[0]), int(r[1])] for r in rows], np.int64).reshape(h, w, 2)
    plane = np.array([[int(x, 16) for x in r[2:6]] for r in rows], np.uint32).view(np.float32).reshape(h, w, 4)
    return src[..., 0], src[..., 1], plane, at + w * h


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """host/overlay_plan_check.cpp built plainly, and once more through `make overlay_asan` (AddressSanitizer + UBSan) in a copy of the
    two directories the rule needs"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("overlay")
    plain = tmp / "overlay_plan_check"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-o", str(plain), str(HOST / "overlay_plan_check.cpp")],
                   check=True)
    work = tmp / "tree" / "nerf-cuda_amd"
    (work / "host").mkdir(parents=True)
    (work / "csrc").mkdir()
    for rel in ("host/Makefile", "host/overlay_plan_check.cpp", "csrc/nrf_overlay_plan.h"):
        shutil.copy(ROOT / "nerf-cuda_amd" / rel, work / rel)
    r = subprocess.run(["make", "-C", str(work / "host"), "overlay_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "-fsanitize=address,undefined" in r.stdout and "-ffp-contract=off" in r.stdout and "overlay_plan_check: 4 cases" in r.stderr + r.stdout
    return plain, work / "host" / "overlay_plan_check", r.stdout


@pytest.fixture(scope="module")
def table():
    return nh.srgb8_table()


# ---------------------------------------------------------------- 1. the declarations
def test_the_header_declares_them_and_the_binding_has_them():
    header = (ROOT / "include" / "nerfhip.h").read_text()
    want = {
        "nrf_rb_srgb8_table": ["float table[256]"],
        "nrf_rb_overlay_image": ["nrf_render_buffer* rb", "float alpha", "const float exposure[3]", "const float background_color[4]",
                                 "int output_color_space", "const void* image", "int image_data_type", "int image_width", "int image_height",
                                 "int fov_axis", "float zoom", "const float screen_center[2]", "void* stream"],
        "nrf_rb_overlay_false_color": ["nrf_render_buffer* rb", "int training_width", "int training_height", "int fov_axis",
                                       "const void* error_map", "int map_width", "int map_height", "const void* average", "float brightness",
                                       "int viridis", "void* stream"],
        "nrf_rb_error_map": ["nrf_render_buffer* rb", "const void* truth_f32x4", "int map_width", "int map_height", "void* error_map",
                             "void* average", "void* stream"],
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
    assert re.search(r"enum\s*\{\s*NRF_IMG_BYTE = 1, NRF_IMG_HALF = 2, NRF_IMG_FLOAT = 3\s*\}", header)
    assert (nh.IMG_BYTE, nh.IMG_HALF, nh.IMG_FLOAT) == (1, 2, 3)
    assert "(csrc/nrf_overlay_plan.h is this text as code.)" in header and "out of scope (NVIDIA" not in (HOST / "render_buffer.h").read_text()
    assert "image-overlay parts of the reference class are out of scope" not in " ".join(header.split())
    assert nh.NRF_ABI_VERSION == 7 == lib.nrf_abi_version()  # additions: no structure changes
    for method in ("overlay_image", "overlay_false_color", "error_map"):
        assert callable(getattr(nh.RenderBuffer, method)), method
    mirror = (HOST / "render_buffer.h").read_text()
    for method in ("overlay_image", "overlay_false_color", "error_map"):
        assert re.search(r"\b" + method + r"\s*\(", mirror), method
    testbed = (HOST / "testbed.cpp").read_text()
    assert '"--overlay_image"' in testbed and '"--overlay_alpha"' in testbed and '"--compare"' in testbed and "error.png" in testbed
    assert re.search(r"^overlay_asan: overlay_plan_check$", (HOST / "Makefile").read_text(), re.M)


def test_the_library_holds_the_overlay_kernels(tmp_path):
    names = hcpu._kernel_names(tmp_path)
    found = sorted(m.group(1) for m in (re.search(r"\boverlay_image_kernel<(\w+)>", n) for n in names) if m)
    assert found == ["1", "2", "3"], found  # one instance per image data type
    for kernel in ("overlay_false_color_kernel", "error_map_kernel", "error_average_kernel"):
        assert any(n.endswith("nrf::" + kernel) for n in names), kernel


def test_the_byte_table_is_the_definition(table):
    """T[b] = srgb_to_linear((float)b * (1.0f / 255.0f)) with libm's power: the replay's decode of the same arguments; monotonic, 0 to 1"""
    assert table.dtype == np.float32 and table.shape == (256,)
    arg = np.arange(256, dtype=np.float32) * (F(1.0) / F(255.0))
    assert np.array_equal(orp.bits(table), orp.bits(orp.decode_srgb(arg)))
    assert table[0] == 0.0 and table[255] == 1.0 and np.all(np.diff(table) > 0)
    with pytest.raises(nh.NerfHipError) as e:
        nh._check(nh.load_library().nrf_rb_srgb8_table(None))
    assert e.value.code == nh.NRF_E_INVALID


# ---------------------------------------------------------------- 2. one text of the definition
def _image_rows():
    """(surface size, image size, type, axis, zoom, centre, alpha, (render, display), curve, exposure): every value of every list of the
    issue's table, the geometry lists crossed in full on every surface, image and type, the colour lists crossed in full on one geometry"""
    rows = []
    k = 0
    for surf in SURFACES:
        for img in IMAGES:
            for ty in TYPES:
                for axis, zoom, center in itertools.product((0, 1), ZOOMS, CENTERS):
                    rows.append((surf, img, ty, axis, zoom, center, ALPHAS[k % 3], SPACES[k % 6], CURVES[k % 4], EXPOSURES[(k // 2) % 3]))
                    k += 1
    for ty in TYPES:  # (in full for Float texels; every third row for the other two types, which differ in read_rgba only)
        for j, (alpha, spaces, curve, exposure) in enumerate(itertools.product(ALPHAS, SPACES, CURVES, EXPOSURES)):
            if ty == nh.IMG_FLOAT or j % 3 == ty:
                rows.append(((19, 11), (7, 5), ty, k % 2, 1.0, (0.5, 0.5), alpha, spaces, curve, exposure))
                k += 1
    return rows


def _image_inputs(k, row):
    surf, img, ty = row[:3]
    bg = [(0.25, 0.5, 1.0, 1.0), (0.9, 0.1, 0.3, 0.5), (0.0, 0.0, 0.0, 0.0)][k % 3]
    return surface_plane(1000 + k, *surf), image_plane(2000 + k, img[0], img[1], ty), bg


def test_the_image_overlay_of_the_plan_header_is_the_replay(programs, table):
    rows = _image_rows()
    assert len(rows) == 2 * 3 * 3 * 30 + 216 + 2 * 72
    inputs = [_image_inputs(k, row) for k, row in enumerate(rows)]
    cases = [image_case(s, im, row[2], row[3], row[7][0], row[7][1], row[8], row[6], row[4], row[5], row[9], bg)
             for row, (s, im, bg) in zip(rows, inputs)]
    want = []
    for row, (s, im, bg) in zip(rows, inputs):
        surf, img, ty, axis, zoom, center, alpha, (rs, ds), curve, exposure = row
        sx, sy = orp.source(surf[0], surf[1], img[0], img[1], axis, zoom, center)
        want.append((sx, sy, orp.overlay_image(s, alpha, exposure, bg, rs, ds, curve, im, ty, table, axis, zoom, center)))
    saturated = off_screen = 0
    for exe in programs[:2]:
        lines, at = run(exe, cases), 0
        for row, (s, _, _), (sx, sy, plane) in zip(rows, inputs, want):
            W, H = row[0]
            gx, gy, got, at = take_pixels(lines, at, W, H)
            assert np.array_equal(gx, sx) and np.array_equal(gy, sy), row
            bad = orp.mismatches(got, plane)
            assert len(bad) == 0, (row, len(bad), bad[:5])
            saturated += int(np.any(np.abs(sx) >= 2 ** 31 - 1))
            if row[5] == (2.0, 2.0) and row[4] in (0.5, 1.0, 3.0):  # the whole image is off screen: prev * (1 - alpha) plus the background
                assert not orp.inside(sx, sy, *row[1]).any(), row
                off_screen += 1
        assert at == len(lines)
    assert saturated >= 2 * 18 * 6 and off_screen >= 2 * 18 * 6  # the zoom of 1e-30 saturates the conversion on every surface


def _false_color_rows():
    rows = []
    k = 0
    for surf in SURFACES:
        # the training resolution: the surface's, half of it, 1.5 times it, and one of another shape (it leaves a border outside the map)
        for tw, th in [surf, (max(1, surf[0] // 2), max(1, surf[1] // 2)), (surf[0] * 3 // 2, surf[1] * 3 // 2), (surf[0], max(1, surf[1] // 2))]:
            for mw, mh in [(1, 1), (3, 2), (16, 16)]:
                for viridis, axis in itertools.product((0, 1), (0, 1)):
                    average = [0.0, np.nan, 0.05, 0.3][k % 4]
                    brightness = [0.0, 16.0, 1.0][k % 3]
                    rows.append((surf, (tw, th), (mw, mh), axis, viridis, average, brightness))
                    k += 1
    return rows


def _false_color_inputs(k, row):
    surf, _, (mw, mh) = row[:3]
    rng = np.random.default_rng(3000 + k)
    emap = rng.uniform(0.0, 0.5, (mh, mw)).astype(np.float32)
    flat = emap.reshape(-1)
    flat[0] = F([-0.5, 2.5, np.nan])[k % 3]           # err below 0, above 1, NaN
    if len(flat) >= 6:
        flat[1], flat[2], flat[3] = -0.5, 2.5, np.nan
    return surface_plane(4000 + k, *surf), emap


def test_the_false_colours_of_the_plan_header_are_the_replay(programs):
    rows = _false_color_rows()
    inputs = [_false_color_inputs(k, row) for k, row in enumerate(rows)]
    cases = [false_color_case(s, row[1][0], row[1][1], row[3], emap, row[5], row[6], row[4]) for row, (s, emap) in zip(rows, inputs)]
    want = []
    for row, (s, emap) in zip(rows, inputs):
        surf, (tw, th), (mw, mh), axis, viridis, average, brightness = row
        want.append((orp.false_color_source(surf[0], surf[1], tw, th, mw, mh, axis), orp.overlay_false_color(s, tw, th, axis, emap, average, brightness, viridis)))
    outside = 0
    for exe in programs[:2]:
        lines, at = run(exe, cases), 0
        for row, (s, _), ((sx, sy), plane) in zip(rows, inputs, want):
            W, H = row[0]
            gx, gy, got, at = take_pixels(lines, at, W, H)
            assert np.array_equal(gx, sx) and np.array_equal(gy, sy), row
            bad = orp.mismatches(got, plane)
            assert len(bad) == 0, (row, len(bad), bad[:5])
            assert np.array_equal(orp.bits(got[..., 3]), orp.bits(s[..., 3]))                 # alpha untouched
            out = ~orp.inside(sx, sy, *row[2])
            assert np.array_equal(orp.bits(got[out]), orp.bits(s[out]))                       # pixels outside the map are left untouched
            outside += int(out.any())
        assert at == len(lines)
    assert outside > 0


# (surface size, map size): exactly one add per lane; lane 0 adds twice; idle lanes; unequal cells; one pixel per cell; a general one;
# two cells of 65 pixels in three rows
ERROR_ROWS = [((64, 1), (1, 1)), ((65, 1), (1, 1)), ((13, 7), (1, 1)), ((13, 7), (5, 3)), ((9, 9), (9, 9)), ((40, 33), (7, 4)), ((130, 3), (2, 1))]


def _error_inputs():
    out = []
    for k, ((W, H), (mw, mh)) in enumerate(ERROR_ROWS):
        s, g = surface_plane(5000 + k, W, H), np.random.default_rng(6000 + k).uniform(0, 1, (H, W, 4)).astype(np.float32)
        s[np.isnan(s) | np.isinf(s)] = 0.5
        out.append((s, g, mw, mh, "finite"))
    s, g = out[3][0].copy(), out[3][1].copy()
    g[4, 7, 1] = np.nan                                       # a plane holding one NaN
    out.append((s, g, 5, 3, "one NaN"))
    out.append((out[5][0], out[5][0].copy(), 7, 4, "identical"))  # an identical truth plane
    return out


def test_the_error_map_of_the_plan_header_is_the_replay(programs):
    inputs = _error_inputs()
    cases = [error_case(s, g, mw, mh) for s, g, mw, mh, _ in inputs]
    want = [orp.error_map(s, g, mw, mh) for s, g, mw, mh, _ in inputs]
    for exe in programs[:2]:
        lines, at = run(exe, cases), 0
        for (s, g, mw, mh, what), (emap, average) in zip(inputs, want):
            assert lines[at] == ["map", "1"]
            got = np.array([int(r[0], 16) for r in lines[at + 1:at + 1 + mw * mh]], np.uint32).view(np.float32).reshape(mh, mw)
            assert lines[at + 1 + mw * mh][0] == "average"
            got_average = np.array([int(lines[at + 1 + mw * mh][1], 16)], np.uint32).view(np.float32)[0]
            at += mw * mh + 2
            assert orp.same(got, emap) and orp.same(got_average, average), (s.shape, mw, mh, what)
            if what == "one NaN":
                assert np.isnan(got).sum() == 1 and np.isnan(got[1, 2]) and np.isnan(got_average)  # pixel (7, 4) lies in cell (2, 1)
            if what == "identical":
                assert not orp.bits(got).any() and orp.bits(got_average) == 0                      # all +0, average +0
            if what == "finite":
                assert np.all(got > 0)
        assert at == len(lines)
        # refused maps: more cells than pixels on an axis, none, more than 512
        s = surface_plane(1, 5, 3)
        for mw, mh in [(6, 1), (1, 4), (0, 1), (1, 0), (-1, 1)]:
            assert run(exe, [error_case(s, s, mw, mh)]) == [["map", "0"]], (mw, mh)
        wide = np.zeros((1, 600, 4), np.float32)
        assert run(exe, [error_case(wide, wide, 513, 1)]) == [["map", "0"]] and run(exe, [error_case(wide, wide, 512, 1)])[0] == ["map", "1"]


def test_the_error_map_is_the_mean_of_the_cell_means():
    """equal cells: the average is the image's mean squared error (to rounding); unequal cells: it is not that, it is the mean of the cells"""
    rng = np.random.default_rng(8)
    s, g = rng.uniform(0, 1, (12, 20, 4)).astype(np.float32), rng.uniform(0, 1, (12, 20, 4)).astype(np.float32)
    mse = np.mean((s[..., :3].astype(np.float64) - g[..., :3]) ** 2)
    emap, average = orp.error_map(s, g, 5, 4)                 # 5 | 20 and 4 | 12
    assert abs(float(average) - mse) <= 1e-6 * mse and abs(float(emap.astype(np.float64).mean()) - mse) <= 1e-6 * mse
    s[:, :2] += 3.0                                           # a bright error in the narrow cells of an unequal split
    mse = np.mean((s[..., :3].astype(np.float64) - g[..., :3]) ** 2)
    emap, average = orp.error_map(s, g, 3, 4)                 # 20 = 7 + 7 + 6 ... columns (0, 7, 14): cells of 7, 7 and 6
    assert list(orp.cell_begins(20, 3)) == [0, 7, 14, 20]
    assert abs(float(average) - float(emap.astype(np.float64).mean())) <= 1e-6 * mse and abs(float(average) - mse) > 1e-3 * mse
    for n, m in [(13, 5), (7, 3), (1031, 512), (521, 512), (16384, 512), (512, 512), (5, 5), (3, 1)]:
        x0 = orp.cell_begins(n, m)
        assert x0[0] == 0 and x0[-1] == n and np.all(np.diff(x0) >= 1)  # every cell holds at least one pixel


# ---------------------------------------------------------------- 3. the replay's pieces against the reference's own kernels
def test_the_byte_table_is_the_references_srgb_to_linear(table):
    import ref_render_buffer_py as rr
    rr.require()
    arg = np.arange(256, dtype=np.float32) * (F(1.0) / F(255.0))
    want = rr.tonemap_color(np.repeat(arg[:, None], 3, axis=1), 0.0, nh.TM_IDENTITY, nh.CS_SRGB, nh.CS_LINEAR)
    for ch in range(3):
        assert np.array_equal(orp.bits(table), orp.bits(want[:, ch]))


def test_the_replays_tonemap_is_the_references_for_per_channel_exposures():
    import ref_render_buffer_py as rr
    rr.require()
    rng = np.random.default_rng(12)
    rgb = rng.uniform(-0.5, 4.0, (400, 3)).astype(np.float32)   # (no NaN and no -0: deviation D-11 is about exactly those)
    for exposure in EXPOSURES + [(-2.0, 2.0, 1.5)]:
        for curve in CURVES:
            for rs, ds in SPACES:
                got = orp.tonemap(rgb, exposure, curve, rs, ds)
                want = rr.tonemap_color(rgb, exposure, curve, rs, ds)
                assert orp.same(got, want), (exposure, curve, rs, ds, orp.mismatches(got, want)[:5])


def test_the_replays_turbo_is_the_references():
    import ref_render_buffer_py as rr
    rr.require()
    x = np.concatenate([np.linspace(-0.5, 1.5, 4001), [np.nan, np.inf, -np.inf, 0.0, 1.0]]).astype(np.float32)
    assert np.array_equal(orp.bits(orp.colormap_turbo(x)), orp.bits(rr.colormap_turbo(x)))


def test_the_replays_pixel_mapping_is_the_references():
    """overlay_depth_kernel shares the mapping: a depth plane whose texel i holds i / n, alpha 1 over a zero surface -- the result's alpha
    is the reference's in-image mask and its colour turbo of the texel the reference chose.  (Without the zoom of 1e-30: the reference's
    bare cast is undefined there.)"""
    import ref_render_buffer_py as rr
    rr.require()
    rows = 0
    for (W, H), (iw, ih) in itertools.product(SURFACES, IMAGES):
        n = iw * ih
        depth = (np.arange(n, dtype=np.float32) / F(n)).reshape(ih, iw)
        colours = orp.colormap_turbo(depth.reshape(-1))
        assert len(np.unique(orp.bits(colours), axis=0)) == n     # a texel is known by its colour
        for axis, zoom, center in itertools.product((0, 1), ZOOMS[:-1], CENTERS):
            got = rr.overlay_depth(np.zeros((H, W, 4), np.float32), 1.0, depth, 1.0, axis, zoom, center)
            sx, sy = orp.source(W, H, iw, ih, axis, zoom, center)
            ok = orp.inside(sx, sy, iw, ih)
            assert np.array_equal(got[..., 3], ok.astype(np.float32)), ((W, H), (iw, ih), axis, zoom, center)
            assert np.array_equal(orp.bits(got[ok][:, :3]), orp.bits(colours[sy[ok] * iw + sx[ok]])), ((W, H), (iw, ih), axis, zoom, center)
            rows += 1
    assert rows == 6 * 2 * 4 * 3


# ---------------------------------------------------------------- 4. the exact consequences of the definition
def test_alpha_zero_returns_the_surfaces_bits(table):
    for k, ty in enumerate(TYPES):
        s = surface_plane(70 + k, 19, 11)
        s[np.isnan(s) | np.isinf(s)] = 0.25
        im = image_plane(80 + k, 7, 5, ty)
        if ty != orp.IMG_BYTE:
            im = image_plane(80 + k, 2, 2, ty)                       # (finite texels: inf * 0 would be a NaN)
        out = orp.overlay_image(s, 0.0, (1.0, -1.0, 2.0), (0.2, 0.4, 0.6, 1.0), k % 3, k % 2, k, im, ty, table, 0, 1.0, (0.5, 0.5))
        assert np.array_equal(out, s) and np.array_equal(orp.bits(np.abs(out)), orp.bits(np.abs(s)))  # (x * 1 + c * 0: the values, -0 + 0 = +0)


def test_alpha_one_with_an_opaque_image_of_the_surfaces_size_returns_the_image(table):
    rng = np.random.default_rng(90)
    im = rng.uniform(0.0, 2.0, (11, 19, 4)).astype(np.float32)
    im[..., 3] = 1.0
    s = surface_plane(91, 19, 11)
    s[np.isnan(s) | np.isinf(s)] = 0.25
    out = orp.overlay_image(s, 1.0, 0.0, (0.3, 0.6, 0.9, 1.0), orp.CS_LINEAR, orp.CS_LINEAR, orp.TM_IDENTITY, im, orp.IMG_FLOAT, table, 0, 1.0, (0.5, 0.5))
    assert np.array_equal(orp.bits(out), orp.bits(im))


def test_the_false_colours_never_change_alpha_and_a_constant_map_scales_the_grey_by_one_colour():
    s = surface_plane(95, 19, 11)
    s[np.isnan(s) | np.isinf(s)] = 0.25
    for viridis in (0, 1):
        emap = np.full((3, 2), 0.2, np.float32)
        out = orp.overlay_false_color(s, 19, 11, 0, emap, 0.1, 1.0, viridis)
        assert np.array_equal(orp.bits(out[..., 3]), orp.bits(s[..., 3]))
        grey = s[..., 0] * F(0.2126) + s[..., 1] * F(0.7152) + s[..., 2] * F(0.0722)
        err = F(0.2) * (F(1.0) / (F(0.0000001) + F(0.1)))
        colour = orp.saturate(orp.colormap_viridis(err * (F(1.0) / (F(1.0) + err))) if viridis else orp.colormap_turbo(err))
        assert colour.shape == (3,) and np.all(colour >= 0) and np.all(colour <= 1) and len(set(colour.tolist())) == 3
        assert np.array_equal(orp.bits(out[..., :3]), orp.bits(grey[..., None] * colour))
