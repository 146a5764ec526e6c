"""nrf_render_rays_clipped, the parts that need no GPU: the checker the GPU tests compare frames with (tests/rays_clip_oracle.py)
pinned to the existing rays oracle, the entry point's place in the ABI and in the Python mirror, and the condition on the GPU
tests' scene that keeps them from passing vacuously (the ramp limit really cuts rays: some partly, some fully, some not at all)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import models
import nerfhip as nh
import oracle_py as op
import rays_clip_oracle as rco
import rays_oracle as ro
import synthetic as syn

W, H = 64, 48
SMALL = {"bound1": dict(), "bound4-cascade3": dict(bound=4.0, cascade=3)}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_scene_cache = {}


def _scene(model):
    """The GPU tests' scene on the oracle, computed once: rays of the orbit camera, the unlimited frame."""
    if model not in _scene_cache:
        desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **SMALL[model])
        orc = op.Oracle(desc)
        o, d, _, _ = orc.generate_rays(syn.default_camera(W, H), syn.orbit_pose(30, 30), W, H)
        full = ro.render(orc, desc, o, d)
        for a in full[:2]:
            a.setflags(write=False)
        _scene_cache[model] = (desc, keep, orc, o, d, full)
    return _scene_cache[model]


@pytest.mark.parametrize("model", list(SMALL))
def test_checker_without_limits_is_the_rays_oracle_bit_for_bit(model):
    desc, keep, orc, o, d, (want, wdepth, wn) = _scene(model)
    n = len(o)
    inf = np.full(n, np.inf, np.float32)
    nan = np.full(n, np.nan, np.float32)
    for what, kw in (("none", dict()), ("-inf / +inf", dict(t_min=-inf, t_max=inf)), ("nan", dict(t_min=nan, t_max=nan)),
                     ("0 / FLT_MAX", dict(t_min=np.zeros(n, np.float32), t_max=np.full(n, ro.FLT_MAX, np.float32)))):
        rgba, depth, ns, raw = rco.render(orc, desc, o, d, **kw)
        assert ns == wn and ns > 1000, what
        assert np.array_equal(_bits(rgba), _bits(want)) and np.array_equal(_bits(depth), _bits(wdepth)), what
        # the raw depth normalises to the depth plane with the epilogue's own arithmetic
        near, far = rco.near_far(desc, o, d, nh.default_options().min_near)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            span = far - near
            dn = np.where(span > 0, np.maximum(raw - near, np.float32(0)) / np.where(span > 0, span, np.float32(1)), np.float32(0))
        assert np.array_equal(_bits(dn), _bits(wdepth)), what
    bgc = nh.default_options()
    bgc.bg_color = 0.25
    want_bg = ro.render(orc, desc, o, d, bgc)
    rgba, depth, _, _ = rco.render(orc, desc, o, d, bgc, background=np.full((n, 3), 0.25, np.float32))
    assert np.array_equal(_bits(rgba), _bits(want_bg[0])) and np.array_equal(_bits(depth), _bits(want_bg[1]))
    assert ro.near_far is not None and ro.near_far.__module__ == "rays_oracle"  # (the wrapper is gone after the call)


def test_clamp_takes_nan_as_no_limit_and_infinities_as_given():
    near, far = np.array([0.2, 0.2, 0.2, 0.2], np.float32), np.array([3.0, 3.0, 3.0, 3.0], np.float32)
    n2, f2 = rco.clamp(near, far, np.array([np.nan, -np.inf, np.inf, 1.0], np.float32), np.array([np.nan, np.inf, -np.inf, 2.0], np.float32))
    assert list(n2) == [np.float32(0.2), np.float32(0.2), np.inf, 1.0]
    assert list(f2) == [3.0, 3.0, -np.inf, 2.0]


def test_render_rays_clipped_is_part_of_the_abi():
    assert "nrf_render_rays_clipped" in nh.exported_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", str(nh.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert {"nrf_render_rays_clipped", "nrf_render_rays"} <= names
    assert nh.load_library().nrf_abi_version() == 7 == nh.NRF_ABI_VERSION
    assert hasattr(nh.NerfHip, "render_rays_clipped") and nh.NRF_RAYS_DEPTH_T == 1
    # the structure as the C compiler lays it out: six 8-byte members and two 4-byte ones
    assert C.sizeof(nh.Rays) == 56
    assert [f[0] for f in nh.Rays._fields_] == ["rays_o", "rays_d", "rays_per_view", "t_min", "t_max", "background", "flags", "reserved"]
    assert nh.Rays.flags.offset == 48 and nh.Rays.reserved.offset == 52


@pytest.mark.parametrize("model", list(SMALL))
def test_the_ramp_cuts_the_gpu_scene_partly_fully_and_not_at_all(model):
    """A condition on the GPU tests' inputs, checked on the oracle alone: as t_max the ramp t(px) = 0.7 + 0.9 px / W leaves pixels
    partly cut, fully cut and untouched; as t_min it leaves pixels partly cut."""
    desc, keep, orc, o, d, (full, fdepth, fn) = _scene(model)
    t = rco.ramp(W, H)
    a_full = full[:, 3]
    hit = a_full > 0
    rgba, depth, n, raw = rco.render(orc, desc, o, d, t_max=t)
    a = rgba[:, 3]
    partly = float(np.mean((a > 0.05) & (a < a_full - 0.05)))
    fully = float(np.mean((a == 0) & (a_full > 0.5)))
    same = np.all(_bits(rgba) == _bits(full), axis=1)  # (rgba: the depth plane is normalised with the ray's own far')
    untouched = float(np.mean(same & hit))
    rgba2, _, n2, _ = rco.render(orc, desc, o, d, t_min=t)
    a2 = rgba2[:, 3]
    partly_min = float(np.mean((a2 > 0.05) & (a2 < a_full - 0.05)))
    print(f"{model}: t_max partly {partly:.3f} fully {fully:.3f} untouched hit pixels {untouched:.3f} samples {n} of {fn}; "
          f"t_min partly {partly_min:.3f} samples {n2}")
    assert partly >= 0.04 and partly_min >= 0.04
    assert fully >= 0.2
    assert untouched >= 0.1
    assert 0 < n < fn and 0 < n2 < fn
