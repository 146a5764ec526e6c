"""nrf_rb_upscale_temporal, nrf_rb_upscale_jitter and nrf_motion_vectors, the parts that need no GPU: the declarations and the bindings,
the kernels' symbols in the built library, the one text of the definition -- host/temporal_plan_check.cpp (csrc/nrf_temporal_plan.h, plain
and under AddressSanitizer + UBSan through `make temporal_asan`) against tests/temporal_replay.py, the numpy replay the GPU tests use, bit
for bit --, the exact consequences of the definition, and what the accumulator is for: from a static camera it beats the spatial
upscaler by at least 2 dB, under a whole-pixel pan by at least 1 dB.  Every test here needs the feature: none passes without it."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import nerfhip as nh
import temporal_replay as tr
import test_ray_hits_cpu as hcpu
import test_upscale_cpu as ucpu
import upscale_replay as ur

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "nerf-cuda_amd" / "host"
F = np.float32
# the issue's rows: ratio 2 (2 x 5 tiles of the kernel), a ragged non-integer ratio, ratio 4, a single texel, the identity
CASES = [((48, 32), (96, 64)), ((40, 30), (53, 41)), ((24, 16), (96, 64)), ((1, 1), (3, 2)), ((31, 17), (31, 17))]


# ---------------------------------------------------------------- 1. the declarations
def test_the_header_declares_them_and_the_binding_has_them():
    header = (ROOT / "include" / "nerfhip.h").read_text()
    want = {
        "nrf_rb_upscale_jitter": ["uint32_t index", "float jitter[2]"],
        "nrf_rb_set_upscale_history": ["nrf_render_buffer* rb", "float max_history"],
        "nrf_rb_upscale_temporal": ["nrf_render_buffer* rb", "const nrf_upscale_temporal* t", "void* rgba8", "void* stream"],
        "nrf_rb_upscale_history": ["nrf_render_buffer* rb", "void** history", "void** weight", "uint32_t* n_frames"],
        "nrf_rb_read_upscale_history": ["nrf_render_buffer* rb", "float* rgba", "float* weight"],
        "nrf_motion_vectors": ["nrf_context* ctx", "const nrf_motion* m", "void* motion_f32x2", "void* stream"],
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
    assert "(csrc/nrf_temporal_plan.h is this text as code.)" in header
    assert re.search(r"enum\s*\{\s*NRF_UPSCALE_T_RESET = 1, NRF_UPSCALE_T_RECTIFY = 2\s*\}", header)
    assert (nh.NRF_UPSCALE_T_RESET, nh.NRF_UPSCALE_T_RECTIFY) == (tr.RESET, tr.RECTIFY) == (1, 2)
    assert nh.NRF_ABI_VERSION == 7 == lib.nrf_abi_version()  # additions: no structure changes
    for method in ("upscale_temporal", "set_upscale_history", "upscale_history", "read_upscale_history"):
        assert callable(getattr(nh.RenderBuffer, method)), method
    assert callable(nh.upscale_jitter) and callable(nh.NerfHip.motion_vectors)
    mirror = (HOST / "render_buffer.h").read_text()
    for method in ("upscale_temporal", "upscale_jitter", "set_upscale_history", "upscale_history_host"):
        assert re.search(r"\b" + method + r"\s*\(", mirror), method
    testbed = (HOST / "testbed.cpp").read_text()
    assert '"--upscale_temporal"' in testbed


def test_the_structures_have_the_headers_layout(tmp_path):
    src = '#include "nerfhip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n", ' \
          'sizeof(nrf_upscale_temporal), offsetof(nrf_upscale_temporal, flags), sizeof(nrf_motion), offsetof(nrf_motion, min_alpha), ' \
          'offsetof(nrf_motion, prev_pose), offsetof(nrf_motion, reserved));return 0;}'
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    sizes = [int(v) for v in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(nh.UpscaleTemporal), nh.UpscaleTemporal.flags.offset, C.sizeof(nh.Motion), nh.Motion.min_alpha.offset,
                     nh.Motion.prev_pose.offset, nh.Motion.reserved.offset]


def test_the_library_holds_the_temporal_kernels(tmp_path):
    names = hcpu._kernel_names(tmp_path)
    found = sorted(m.group(1).replace(" ", "") for m in (re.search(r"\btemporal_kernel<([\w, ]+)>", n) for n in names) if m)
    assert found == ["false,false", "false,true", "true,false", "true,true"], found  # {packed 8-bit plane} x {motion plane}
    assert any(re.search(r"\bmotion_kernel\b", n) for n in names)


def test_the_jitter_call_is_host_only_and_is_the_replay():
    for k in list(range(40)) + [1000, 2**31, 2**32 - 1]:
        got = nh.upscale_jitter(k)
        want = tr.jitter(k)
        assert np.array_equal(ur.bits(F(got)), ur.bits(F(want))), k
    assert nh.load_library().nrf_rb_upscale_jitter(0, None) == nh.NRF_E_INVALID


# ---------------------------------------------------------------- 2. one text of the definition
def _hex(a):
    return " ".join(f"{w:08x}" for w in ur.bits(a).reshape(-1))


def _motion_plane(seed, iw, ih, ow, oh):
    """zero, whole, fractional, out-of-plane, +inf and NaN vectors, a -0 among the zeros"""
    rng = np.random.default_rng(seed)
    m = np.zeros((ih, iw, 2), np.float32)
    kind = rng.integers(0, 6, (ih, iw))
    m[kind == 1] = rng.integers(-3, 4, (ih, iw, 2)).astype(np.float32)[kind == 1]
    m[kind == 2] = rng.uniform(-2.5, 2.5, (ih, iw, 2)).astype(np.float32)[kind == 2]
    m[kind == 3] = (rng.choice([-1.0, 1.0], (ih, iw, 2)) * [ow + 2, oh + 2]).astype(np.float32)[kind == 3]
    m[kind == 4] = F(np.inf)
    m[kind == 5] = rng.uniform(-0.75, 0.75, (ih, iw, 2)).astype(np.float32)[kind == 5]
    flat = m.reshape(-1, 2)
    flat[0] = [F(-0.0), F(0.0)]
    if len(flat) > 3:
        flat[1], flat[2], flat[3] = [F(np.nan), F(0.0)], [F(0.0), F(1.0)], [F(0.5), F(-0.5)]
    return m


def _run_temporal(exe, frames, ow, oh, amount, max_history):
    """frames: [(plane, jitter, flags, motion or None)] -> per frame uint32 [oh][ow][10], or None for a refused plan"""
    ih, iw = frames[0][0].shape[:2]
    text = [f"T {iw} {ih} {ow} {oh} {_hex(F(amount))} {_hex(F(max_history))} {len(frames)}"]
    for plane, jitter, flags, motion in frames:
        text.append(f"{_hex(F(jitter[0]))} {_hex(F(jitter[1]))} {flags} {0 if motion is None else 1}")
        text.append(_hex(plane))
        if motion is not None:
            text.append(_hex(motion))
    out = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    if lines[0].split()[1] == "0" or lines[-1] == "plan 0":
        return None
    words = np.array([int(w, 16) for ln in lines[1:] for w in ln.split()], np.uint32).reshape(len(frames), oh, ow, 10)
    return [int(w, 16) for w in lines[0].split()[2:]], words


def _frames(case, seed, with_motion, flags):
    (iw, ih), (ow, oh) = case
    jitters = [(0.0, 0.0), tr.jitter(1), (0.5, -0.5)]
    return [(ucpu._plane(seed + k, iw, ih), jitters[k], flags[k], _motion_plane(seed + 10 + k, iw, ih, ow, oh) if with_motion else None)
            for k in range(3)]


# (a motion plane?, the three frames' flags): the static path; motion with and without the clamp; a reset in the middle, then both flags
RUNS = [(False, (0, 0, tr.RECTIFY)), (True, (0, tr.RECTIFY, 0)), (True, (tr.RECTIFY, tr.RESET, tr.RESET | tr.RECTIFY)),
        (True, (0, 0, tr.RECTIFY))]


def _replay(frames, ow, oh, amount, max_history):
    T = tr.Temporal(ow, oh, amount, max_history)
    out = []
    for plane, jitter, flags, motion in frames:
        shown, packed = T.step(plane, jitter, motion, flags)
        out.append((T.H.copy(), T.Wt.copy(), shown, packed))
    return out


def _same(words, want, what):
    H, Wt, shown, packed = want
    for name, got, ref in (("H'", words[..., 0:4], ur.bits(H)), ("Wt'", words[..., 4], ur.bits(Wt)), ("presented", words[..., 5:9], ur.bits(shown)),
                           ("rgba8", words[..., 9], packed)):
        bad = np.nonzero(got != ref)
        assert len(bad[0]) == 0, (what, name, len(bad[0]), [b[:5] for b in bad])


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """host/temporal_plan_check.cpp built plainly, and once more through `make temporal_asan` (AddressSanitizer + UBSan) in a copy of the
    two directories the rule needs"""
    tmp_path = tmp_path_factory.mktemp("temporal")
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    plain = tmp_path / "temporal_plan_check"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-o", str(plain), str(HOST / "temporal_plan_check.cpp")], check=True)
    work = tmp_path / "tree" / "nerf-cuda_amd"
    (work / "host").mkdir(parents=True)
    (work / "csrc").mkdir()
    for rel in ("host/Makefile", "host/temporal_plan_check.cpp", "csrc/nrf_temporal_plan.h", "csrc/nrf_upscale_plan.h"):
        shutil.copy(ROOT / "nerf-cuda_amd" / rel, work / rel)
    r = subprocess.run(["make", "-C", str(work / "host"), "temporal_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "-fsanitize=address,undefined" in r.stdout and "-ffp-contract=off" in r.stdout and "2 x 2 -> 3 x 4, 2 frames" in r.stderr + r.stdout
    assert re.search(r"^temporal_asan: temporal_plan_check$", (HOST / "Makefile").read_text(), re.M)
    return plain, work / "host" / "temporal_plan_check"


@pytest.mark.parametrize("case", CASES)
def test_the_plan_header_and_the_numpy_replay_are_one_definition(programs, case):
    """three frames per run -- H', Wt', the presented plane and the packed dwords of every frame, bit for bit"""
    (iw, ih), (ow, oh) = case
    for k, (with_motion, flags) in enumerate(RUNS):
        amount, max_history = (0.0, 0.5, 2.0, 0.25)[k], (64.0, 1.0, 256.0, 2.5)[k]
        frames = _frames(case, 700 + 31 * k + iw, with_motion, flags)
        assert (frames[0][0] < 0).any() and (frames[0][0] > 1).any()
        want = _replay(frames, ow, oh, amount, max_history)
        for exe in programs:
            head, words = _run_temporal(exe, frames, ow, oh, amount, max_history)
            assert head == [int(ur.bits(v).reshape(-1)[0]) for v in (F(iw) / F(ow), F(ih) / F(oh), F(ow) / F(iw), F(oh) / F(ih))]
            for f in range(3):
                _same(words[f], want[f], (case, k, f))
        if with_motion and iw > 1:                                 # the plane did take every path
            m = frames[1][3]
            assert np.isinf(m).any() and (m == 0).all(axis=2).any() and (np.abs(m) > ow).any() and (m != np.floor(m)).any()


def test_refused_plans(programs):
    one = ucpu._plane(1, 1, 1)
    for exe in programs:
        for (ow, oh), amount, max_history, jitter, flags in [((0, 1), 0.0, 64.0, (0, 0), 0), ((9, 1), 0.0, 64.0, (0, 0), 0), ((8, 8), 2.5, 64.0, (0, 0), 0),
                                                             ((8, 8), 0.0, 0.5, (0, 0), 0), ((8, 8), 0.0, 257.0, (0, 0), 0), ((8, 8), 0.0, np.nan, (0, 0), 0),
                                                             ((8, 8), 0.0, 64.0, (0.51, 0), 0), ((8, 8), 0.0, 64.0, (0, -0.75), 0),
                                                             ((8, 8), 0.0, 64.0, (np.nan, 0), 0), ((8, 8), 0.0, 64.0, (0, np.inf), 0),
                                                             ((8, 8), 0.0, 64.0, (0, 0), 4)]:
            assert _run_temporal(exe, [(one, jitter, flags, None)], ow, oh, amount, max_history) is None, (ow, oh, amount, max_history, jitter, flags)
        assert _run_temporal(exe, [(one, (0.5, -0.5), 3, None)], 8, 8, 2.0, 256.0) is not None


# ---------------------------------------------------------------- 3. the exact consequences of the definition
def test_a_reset_frame_without_jitter_is_the_spatial_upscaler_bit_for_bit():
    for k, ((iw, ih), (ow, oh)) in enumerate(CASES):
        plane = ucpu._plane(800 + k, iw, ih)
        for amount in (0.0, 0.5, 2.0):
            want, packed = ur.upscale(plane, ow, oh, amount)
            T = tr.Temporal(ow, oh, amount)
            got, got8 = T.step(plane)                                             # the first frame
            assert np.array_equal(ur.bits(got), ur.bits(want)) and np.array_equal(got8, packed)
            T.step(ucpu._plane(900 + k, iw, ih), tr.jitter(3))
            got, got8 = T.step(plane, (0.0, 0.0), None, tr.RESET)                 # a reset over a history
            assert np.array_equal(ur.bits(got), ur.bits(want)) and np.array_equal(got8, packed)
            assert np.array_equal(ur.bits(T.H), ur.bits(ur.reconstruct(plane, ow, oh)))


def test_a_constant_plane_stays_constant_over_eight_jittered_frames():
    texel = F([0.3, -1.7, 2.5, 1e-3])
    for (iw, ih), (ow, oh) in CASES:
        plane = np.broadcast_to(texel, (ih, iw, 4)).copy()
        for flags, motion in ((0, None), (tr.RECTIFY, None), (0, _motion_plane(5, iw, ih, ow, oh)), (tr.RECTIFY, _motion_plane(6, iw, ih, ow, oh))):
            T = tr.Temporal(ow, oh, 0.5)
            for k in range(8):
                out, packed = T.step(plane, tr.jitter(k), motion, flags)
                assert np.array_equal(ur.bits(out), np.broadcast_to(ur.bits(texel), (oh, ow, 4))), ((iw, ih), (ow, oh), flags, k)
                assert np.array_equal(ur.bits(T.H), np.broadcast_to(ur.bits(texel), (oh, ow, 4)))
                assert np.all(packed == ur.rgba8(texel))


def test_where_the_vector_leaves_the_plane_or_is_infinite_the_pixel_is_reset():
    (iw, ih), (ow, oh) = (24, 16), (96, 64)
    motion = np.zeros((ih, iw, 2), np.float32)
    motion[:, 0:6] = F(np.inf)
    motion[:, 6:12] = F([200.0, 0.0])
    motion[:, 12:18] = F([0.0, -65.0])
    motion[:, 18:24] = F([0.25, 0.5])                                            # stays inside (except at the border)
    planes = [ucpu._plane(40 + k, iw, ih) for k in range(3)]
    T, R = tr.Temporal(ow, oh, 0.0), tr.Temporal(ow, oh, 0.0)
    T.step(planes[0])
    T.step(planes[1], tr.jitter(1), motion)
    j = tr.jitter(2)
    out, _ = T.step(planes[2], j, motion)
    ref, _ = R.step(planes[2], j, None, tr.RESET)
    _, _, nx, _ = tr.current(planes[2], ow, oh, j)
    gone = np.broadcast_to((nx < 18)[None, :], (oh, ow))
    assert np.array_equal(ur.bits(T.H)[gone], ur.bits(R.H)[gone]) and np.array_equal(ur.bits(T.Wt)[gone], ur.bits(R.Wt)[gone])
    inside = np.broadcast_to((nx >= 18)[None, :], (oh, ow)).copy()
    inside[:, -2:] = False
    inside[-2:, :] = False
    assert np.all(T.Wt[inside] > R.Wt[inside]) and not np.array_equal(T.H[inside], R.H[inside])


def test_the_weight_never_exceeds_the_history_length_plus_one():
    (iw, ih), (ow, oh) = (40, 30), (53, 41)
    plane = ucpu._plane(3, iw, ih)
    for max_history in (1.0, 4.0, 64.0):
        T = tr.Temporal(ow, oh, 0.0, max_history)
        for k in range(200 if max_history == 64.0 else 16):
            T.step(plane, tr.jitter(k))
            assert np.all(T.Wt <= F(max_history) + F(1.0)) and np.all(T.Wt >= tr.WEIGHT_FLOOR)
        assert T.Wt.max() > max_history                                           # the cap was reached


def test_the_jitter_sequence():
    # halton2 is exact: the bit-reversed index; the first 8 points by hand
    for k in range(1, 4096):
        assert float(tr.halton(k, 2)) == int(format(k, "012b")[::-1], 2) / 4096.0
    third = [1 / 3, 2 / 3, 1 / 9, 4 / 9, 7 / 9, 2 / 9, 5 / 9, 8 / 9]
    half = [1 / 2, 1 / 4, 3 / 4, 1 / 8, 5 / 8, 3 / 8, 7 / 8, 1 / 16]
    for k in range(8):
        jx, jy = tr.jitter(k)
        assert float(jx) == half[k] - 0.5 and abs(float(jy) - (third[k] - 0.5)) < 1e-6, k
    for k in range(20000):
        jx, jy = tr.jitter(k)
        assert -0.5 <= jx < 0.5 and -0.5 <= jy < 0.5 and jx.dtype == jy.dtype == np.float32


def test_the_fractions_and_the_indices_stay_in_range_under_any_jitter():
    rng = np.random.default_rng(12)
    sizes = [(1, 1), (1, 8), (2, 16), (540, 1080), (2048, 16384), (16383, 16384), (16384, 16384), (5461, 16383)]
    for _ in range(60):
        n_in = int(rng.integers(1, 16385))
        sizes.append((n_in, int(rng.integers(n_in, min(8 * n_in, 16384) + 1))))
    for n_in, n_out in sizes:
        for j in (-0.5, 0.5, 0.0, float(rng.uniform(-0.5, 0.5)), 2.0 ** -26, -(2.0 ** -26)):
            taps, w, n, d = tr._axis(n_in, n_out, j)
            base = taps[:, 1]
            assert taps.min() >= 0 and taps.max() <= n_in - 1 and np.all(np.diff(base) >= 0), (n_in, n_out, j)
            assert np.all(n >= 0) and np.all(n <= n_in - 1)
            # the nearest texel and its neighbours lie within the taps' range: what the kernel's LDS image holds
            assert np.all(np.clip(n - 1, 0, n_in - 1) >= taps[:, 0]) and np.all(np.clip(n + 1, 0, n_in - 1) <= taps[:, 3]), (n_in, n_out, j)
            # a tile's footprint: 64 apron columns span at most 70 source texels
            if n_out > 64:
                assert (taps[63:, 3] - taps[:-63, 0]).max() + 1 <= 70, (n_in, n_out, j)
            assert np.all(np.isfinite(w)) and np.all(np.isfinite(d))


# ---------------------------------------------------------------- 4. what the accumulator is for
def _analytic(w, h, off=(0.0, 0.0), scale=(1.0, 1.0), shift=(0.0, 0.0)):
    """the analytic image of tests/test_upscale_cpu.py (four channels, the disc the finest) sampled at ((x + 0.5 + off) * scale + shift) / w"""
    x = (((np.arange(w) + 0.5 + off[0]) * scale[0] + shift[0]) / (w * scale[0]))[None, :]
    y = (((np.arange(h) + 0.5 + off[1]) * scale[1] + shift[1]) / (h * scale[1]))[:, None]
    wave = 0.5 + 0.5 * np.sin(9 * x + 4 * y) * np.cos(7 * y - 2 * x)
    edge = 1.0 / (1.0 + np.exp(-40.0 * (0.8 * x + 0.6 * y - 0.7)))
    ring = np.exp(-0.5 * ((np.hypot(x - 0.5, y - 0.45) - 0.3) / 0.04) ** 2)
    disc = 1.0 / (1.0 + np.exp(60.0 * (np.hypot(x - 0.5, y - 0.5) - 0.4)))
    return np.stack([wave, edge, ring, disc], axis=2)


def test_the_jittered_image_is_the_upscale_tests_image():
    assert np.array_equal(_analytic(48, 32), ucpu._analytic(48, 32))


def _static(src, dst, n_frames=16, flags=0):
    T = tr.Temporal(dst[0], dst[1], 0.0, 64.0)
    for k in range(n_frames):
        j = (F(0), F(0)) if k == 0 else tr.jitter(k)
        T.step(_analytic(*src, off=(float(j[0]), float(j[1]))).astype(np.float32), j, None, flags)
    return T.H


@pytest.mark.parametrize("src,dst", [((48, 32), (96, 64)), ((48, 32), (72, 48)), ((40, 30), (53, 41)), ((24, 16), (96, 64))])
def test_sixteen_jittered_frames_beat_the_spatial_upscaler_by_two_decibels(src, dst):
    high = _analytic(*dst)
    base = ucpu._psnr(ur.reconstruct(_analytic(*src).astype(np.float32), *dst), high)
    got = ucpu._psnr(_static(src, dst), high)
    clamped = ucpu._psnr(_static(src, dst, flags=tr.RECTIFY), high)
    print(f"{src} -> {dst}: temporal {got:.2f} dB against spatial {base:.2f} dB (+{got - base:.2f}); rectified {clamped:.2f} dB ({clamped - got:+.2f})")
    assert got >= base + 2.0, (src, dst, got, base)


def test_the_gain_at_equal_resolutions_is_printed():
    src = dst = (48, 32)
    high = _analytic(*dst)
    base = ucpu._psnr(ur.reconstruct(_analytic(*src).astype(np.float32), *dst), high)
    got = ucpu._psnr(_static(src, dst), high)
    print(f"{src} -> {dst}: temporal {got:.2f} dB against spatial {base:.2f} dB (the identity: nothing can beat it)")
    assert np.isfinite(got)


def _pan(src, dst, speed, flags=0, n_frames=16):
    """a camera panning by `speed` output pixels per frame along x: frame k shows the image shifted by k * speed output pixels, and every
    motion vector is (speed, 0).  -> (PSNR of the history, PSNR of the spatial upscaler on the last frame rendered without jitter)"""
    (iw, ih), (ow, oh) = src, dst
    scale = (ow / iw, oh / ih)
    motion = np.broadcast_to(F([speed, 0.0]), (ih, iw, 2)).copy()
    T = tr.Temporal(ow, oh, 0.0, 64.0)
    for k in range(n_frames):
        j = (F(0), F(0)) if k == 0 else tr.jitter(k)
        frame = _analytic(iw, ih, off=(float(j[0]), float(j[1])), scale=scale, shift=(k * speed, 0.0)).astype(np.float32)
        T.step(frame, j, motion, flags)
    last = (n_frames - 1) * speed
    truth = _analytic(ow, oh, shift=(last, 0.0))
    spatial = ur.reconstruct(_analytic(iw, ih, scale=scale, shift=(last, 0.0)).astype(np.float32), ow, oh)
    return ucpu._psnr(T.H, truth), ucpu._psnr(spatial, truth)


@pytest.mark.parametrize("src,dst", [((48, 32), (96, 64)), ((24, 16), (96, 64))])
def test_a_pan_by_one_output_pixel_per_frame_beats_the_spatial_upscaler_by_one_decibel(src, dst):
    got, base = _pan(src, dst, 1.0)
    print(f"{src} -> {dst}, pan 1 px/frame: temporal {got:.2f} dB against spatial {base:.2f} dB (+{got - base:.2f})")
    assert got >= base + 1.0, (src, dst, got, base)


def test_the_fractional_pans_are_printed():
    """repeated resampling of the history loses detail: recorded in DESIGN.md, not asserted"""
    for src, dst in [((48, 32), (96, 64)), ((24, 16), (96, 64))]:
        for speed in (0.5, 1.25):
            got, base = _pan(src, dst, speed)
            clamped, _ = _pan(src, dst, speed, flags=tr.RECTIFY)
            print(f"{src} -> {dst}, pan {speed} px/frame: temporal {got:.2f} dB, rectified {clamped:.2f} dB, spatial {base:.2f} dB")
            assert np.isfinite(got) and np.isfinite(clamped)


# ---------------------------------------------------------------- 5. the motion vectors
def _pose(angle, height, radius=2.5):
    """a camera on a circle looking at the origin (columns: right, up, back; the position)"""
    eye = np.array([radius * np.cos(angle), radius * np.sin(angle), height])
    back = eye / np.linalg.norm(eye)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    p = np.eye(4)
    p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = right, up, back, eye
    return p.astype(np.float32)


def _rays(w, h, cam, pose, scale):
    """the rays of a pinhole camera in the library's convention, as values (the tests below need rays, not these bits)"""
    R, c, cam = tr.camera(pose, scale, cam)
    xs = ((np.arange(w) + 0.5 - cam[2]) / cam[0])[None, :] + np.zeros((h, 1))
    ys = ((np.arange(h) + 0.5 - cam[3]) / cam[1])[:, None] + np.zeros((1, w))
    v = np.stack([xs, ys, np.ones((h, w))], axis=2)
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    d = (v @ R.astype(np.float64).T).astype(np.float32)
    return np.broadcast_to(c, (h, w, 3)).copy(), d


def _scene(w, h, seed):
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    t = rng.uniform(0.5, 3.0, (h, w)).astype(np.float32)
    return alpha, (alpha * t).astype(np.float32)


def _run_motion(exe, o, d, alpha, depth, ow, oh, min_alpha, scale, cam, pose, prev_cam, prev_pose):
    h, w = alpha.shape
    rows = np.concatenate([o.reshape(-1, 3), d.reshape(-1, 3), alpha.reshape(-1, 1), depth.reshape(-1, 1)], axis=1).astype(np.float32)
    text = f"M {w} {h} {ow} {oh} {_hex(F(min_alpha))} {_hex(F(scale))}\n{_hex(pose)} {_hex(cam)}\n{_hex(prev_pose)} {_hex(prev_cam)}\n{_hex(rows)}\n"
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    if lines[0] == "plan 0":
        return None
    return np.array([int(v, 16) for ln in lines[1:] for v in ln.split()], np.uint32).reshape(h, w, 2)


W, H, OW, OH, SCALE = 40, 30, 53, 41, 0.33
CAM = F([45.0, 44.0, 20.25, 14.5])


def test_the_motion_vectors_of_the_check_program_are_the_replays(programs):
    pose, prev_pose = _pose(0.4, 1.0), _pose(0.47, 1.1)
    prev_cam = CAM + F([1.0, -0.5, 0.75, 0.25])
    o, d = _rays(W, H, CAM, pose, SCALE)
    alpha, depth = _scene(W, H, 1)
    alpha[0, :4] = F([0.0, np.nan, 0.25, 1.0])
    depth[1, :4] = F([np.inf, np.nan, -1.0, 0.0])
    d[2, 0], o[2, 1, 1], d[2, 2] = F(np.nan), F(np.inf), -d[2, 2]                # rays that are not finite; one that looks backwards
    want = tr.motion_vectors(o, d, alpha, depth, OW, OH, 0.5, tr.camera(pose, SCALE, CAM), tr.camera(prev_pose, SCALE, prev_cam))
    assert np.isinf(want[2, :3]).all() and np.isfinite(want[5:]).all() and np.abs(want[5:]).max() > 1
    for exe in programs:
        got = _run_motion(exe, o, d, alpha, depth, OW, OH, 0.5, SCALE, CAM, pose, prev_cam, prev_pose)
        bad = np.nonzero(got != ur.bits(want))
        assert len(bad[0]) == 0, (len(bad[0]), [b[:5] for b in bad])
        for min_alpha in (0.0, -0.5, 1.5, np.nan):
            assert _run_motion(exe, o, d, alpha, depth, OW, OH, min_alpha, SCALE, CAM, pose, prev_cam, prev_pose) is None
        assert _run_motion(exe, o, d, alpha, depth, W - 1, OH, 0.5, SCALE, CAM, pose, prev_cam, prev_pose) is None


def test_identical_cameras_give_exactly_zero():
    pose = _pose(1.1, 0.7)
    o, d = _rays(W, H, CAM, pose, SCALE)
    alpha, depth = _scene(W, H, 2)
    K = tr.camera(pose, SCALE, CAM)
    m = tr.motion_vectors(o, d, alpha, depth, OW, OH, 0.5, K, K)
    assert (alpha < 0.5).any() and (alpha >= 0.5).any()                           # both the points and the directions
    assert np.all(m == 0)
    # ... also for the rays of a jittered camera: both projections go through the unjittered one
    o, d = _rays(W, H, CAM - F([0, 0, 0.3, -0.2]), pose, SCALE)
    assert np.all(tr.motion_vectors(o, d, alpha, depth, OW, OH, 0.5, K, K) == 0)


def test_a_principal_point_two_pixels_further_moves_every_pixel_by_two_render_pixels():
    pose = _pose(2.0, 0.3)
    o, d = _rays(W, H, CAM, pose, SCALE)
    alpha, depth = _scene(W, H, 3)
    m = tr.motion_vectors(o, d, alpha, depth, OW, OH, 0.5, tr.camera(pose, SCALE, CAM), tr.camera(pose, SCALE, CAM + F([0, 0, 2, 0])))
    assert np.abs(m[..., 0] - 2.0 * OW / W).max() <= 1e-3 and np.all(m[..., 1] == 0)


def test_a_point_behind_the_previous_camera_has_no_history():
    pose = _pose(0.0, 0.0)
    o, d = _rays(W, H, CAM, pose, SCALE)
    alpha = np.ones((H, W), np.float32)
    depth = np.full((H, W), 0.5, np.float32)                                      # points half a unit in front of the camera ...
    prev = pose.copy()
    prev[:3, 3] = pose[:3, 3] - pose[:3, 2] * F(3.0)                              # ... and the previous camera beyond them, looking the same way
    m = tr.motion_vectors(o, d, alpha, depth, OW, OH, 0.5, tr.camera(pose, SCALE, CAM), tr.camera(prev, SCALE, CAM))
    assert np.all(np.isposinf(m))
    alpha[:] = 0.1                                                                # at infinity the translation is ignored: exactly zero
    assert np.all(tr.motion_vectors(o, d, alpha, depth, OW, OH, 0.5, tr.camera(pose, SCALE, CAM), tr.camera(prev, SCALE, CAM)) == 0)
