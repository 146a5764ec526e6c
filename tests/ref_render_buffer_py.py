"""ctypes binding of oracle/_ref/libref_render_buffer.so -- TEST INFRASTRUCTURE ONLY.

The library is the reference's own render-buffer kernels compiled for the CPU (oracle/ref_render_buffer.cpp, `make -C oracle ref`):
accumulate_kernel, tonemap_kernel with its two `tonemap` functions, colormap_turbo and overlay_depth_kernel, each launched with
the geometry of its call site in CudaRenderBuffer.  It needs a reference tree at build time and is never committed; `require()`
fails where the tree exists and the library does not, and skips where neither exists (ref_kernels_py.require's rule; the committed
vectors of tests/golden/reference_render_buffer.npz stand in on such a machine, tests/test_reference_render_buffer_gpu.py).

Planes are float32 [H][W][4]; colour spaces and curves are nerfhip.h's numbers, which `lib()` asserts are the reference's."""
from __future__ import annotations

import ctypes as C

import numpy as np

import ref_kernels_py as rk

LIB = rk.ROOT / "oracle" / "_ref" / "libref_render_buffer.so"
_lib = None

# nerfhip.h's NRF_CS_* / NRF_TM_* -> the reference's enumerator
COLOR_SPACES = {0: "EColorSpace::Linear", 1: "EColorSpace::SRGB", 2: "EColorSpace::VisPosNeg"}
CURVES = {0: "ETonemapCurve::Identity", 1: "ETonemapCurve::ACES", 2: "ETonemapCurve::Hable", 3: "ETonemapCurve::Reinhard"}


def require():
    """The loaded library; a pytest failure where it should exist and does not, a skip where it cannot."""
    import pytest

    if not LIB.exists():
        if rk.reference_tree_exists():
            pytest.fail(f"{LIB} is missing although the reference tree {rk.REFERENCE} exists: run `make -C oracle ref` (build() does)")
        pytest.skip("no reference tree and no oracle/_ref/libref_render_buffer.so: nothing to hold the oracle's render buffer to on this machine")
    return lib()


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = C.CDLL(str(LIB))
    vp, u32, i32, f32 = C.c_void_p, C.c_uint32, C.c_int, C.c_float
    sig = {
        "refrb_enum_value": (i32, [C.c_char_p]),
        "refrb_accumulate": (None, [i32, i32, vp, vp, f32, i32]),
        "refrb_tonemap": (None, [i32, i32, f32, vp, vp, i32, i32, i32, i32, vp]),
        "refrb_film_curve": (None, [u32, vp, i32, vp]),
        "refrb_tonemap_color": (None, [u32, vp, vp, i32, i32, i32, vp]),
        "refrb_colormap_turbo": (None, [u32, vp, vp]),
        "refrb_overlay_depth": (None, [i32, i32, f32, vp, f32, i32, i32, i32, f32, f32, f32, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    for table in (COLOR_SPACES, CURVES):
        for number, name in table.items():
            assert L.refrb_enum_value(name.encode()) == number, f"{name} is not {number} in the reference"
    _lib = L
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return a.ctypes.data


def _plane(a):
    a = _f32(a)
    assert a.ndim == 3 and a.shape[2] == 4, "planes are [H][W][4]"
    return a


def accumulate(frame, accum, sample_count, color_space):
    """accumulate_kernel as CudaRenderBuffer::accumulate launches it: the new accumulate plane"""
    frame, accum = _plane(frame), _plane(accum).copy()
    H, W = frame.shape[:2]
    lib().refrb_accumulate(W, H, _p(frame), _p(accum), float(sample_count), color_space)
    return accum


def tonemap(accum, exposure, bg, color_space, output_color_space, curve, clamp=False):
    """tonemap_kernel as CudaRenderBuffer::tonemap launches it: the surface"""
    accum, bg = _plane(accum), _f32(bg).reshape(4)
    H, W = accum.shape[:2]
    out = np.full_like(accum, 777.0)  # every texel is written
    lib().refrb_tonemap(W, H, float(exposure), _p(bg), _p(accum), color_space, output_color_space, curve, int(clamp), _p(out))
    return out


def film_curve(rgb, curve):
    """tonemap(x, curve) on colours [n][3]"""
    rgb = _f32(rgb).reshape(-1, 3)
    out = np.empty_like(rgb)
    lib().refrb_film_curve(len(rgb), _p(rgb), curve, _p(out))
    return out


def tonemap_color(rgb, exposure, curve, color_space, output_color_space):
    """tonemap(col, exposure, curve, color_space, output_color_space) on colours [n][3]; exposure: one value or three"""
    rgb = _f32(rgb).reshape(-1, 3)
    e = _f32(np.broadcast_to(np.asarray(exposure, np.float32), (3,)))
    out = np.empty_like(rgb)
    lib().refrb_tonemap_color(len(rgb), _p(rgb), _p(e), curve, color_space, output_color_space, _p(out))
    return out


def colormap_turbo(x):
    x = _f32(x).reshape(-1)
    out = np.empty((len(x), 3), np.float32)
    lib().refrb_colormap_turbo(len(x), _p(x), _p(out))
    return out


def overlay_depth(surface, alpha, depth, depth_scale, fov_axis, zoom, center):
    """overlay_depth_kernel as CudaRenderBuffer::overlay_depth launches it, in oracle_py.rb_overlay_depth's form"""
    surface, depth = _plane(surface).copy(), _f32(depth)
    H, W = surface.shape[:2]
    ih, iw = depth.shape
    lib().refrb_overlay_depth(W, H, float(alpha), _p(depth), float(depth_scale), iw, ih, int(fov_axis), float(zoom), float(center[0]),
                              float(center[1]), _p(surface))
    return surface
