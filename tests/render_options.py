"""The nrf_options rows every rendering entry point is held to -- TEST INFRASTRUCTURE ONLY (no test in it).

One table, imported by tests/test_render_rays_cpu.py (the checker under every row, and the condition that a row moves the
frame) and tests/test_render_options_gpu.py (every ray entry point and stage under the rows).  A row is a dict of nrf_options
fields; "min_near_beyond_far" depends on the model's bound and is resolved by options().  No non-finite or negative value is
listed: nrf_set_options does not refuse them, and what the kernels do with them is not held to anything.

    ROWS         rows that change the picture: a twin test under one of them must also show that the row moved the frame (moved)
    EXACT_ROWS   rows whose frame is known without a network: density_scale 0 composites weight 0 from every march sample -- the
                 frame is the background, alpha and depth 0, and n_composited counts the march alone --; a min_near beyond every
                 ray's far leaves no ray alive
    REDUCED      the rows the stage and march-form instances are run under
"""
from __future__ import annotations

import numpy as np

import nerfhip as nh

ROWS = {
    "density_scale0.37": dict(density_scale=0.37),
    "density_scale2": dict(density_scale=2.0),
    "max_steps1": dict(max_steps=1),
    "max_steps7": dict(max_steps=7),
    "min_near0.05": dict(min_near=0.05),
    "dt_gamma0": dict(dt_gamma=0.0),
    "dt_gamma1_32": dict(dt_gamma=1.0 / 32.0),
    "bg0.25": dict(bg_color=0.25),
    # the row of tests/test_parity_gpu.py::test_render_options_and_multilevel_scene
    "combined": dict(bg_color=0.25, density_scale=0.5, max_steps=64, min_near=0.05),
}
# min_near beyond every ray's far: the box's diagonal is 2 sqrt(3) bound (3.47 / 13.9), but a camera outside the box at the orbit
# radius leaves less than that; 3.2 and 9.0 exceed every far of the frames used (asserted on the oracle, test_render_rays_cpu.py)
BEYOND_FAR = {1.0: 3.2, 4.0: 9.0}
EXACT_ROWS = {
    "density_scale0": dict(density_scale=0.0),
    "density_scale0-max_steps37": dict(density_scale=0.0, max_steps=37),
    "min_near_beyond_far": dict(min_near=BEYOND_FAR),
}
ALL_ROWS = {**ROWS, **EXACT_ROWS}
REDUCED = ["density_scale0.37", "max_steps7", "min_near0.05", "dt_gamma0", "combined"]
THRESHOLD = 8.0 / 255.0
# moved() must reach this for a row: the share of the pixels the default frame touches; "bg0.25" moves the pixels the object does
# NOT cover and is held over all pixels; "max_steps1" to half of what the oracle gives at the weakest shape (0.982 .. 0.984 at both
# hot models, 64 x 48 and 33 x 70: test_render_rays_cpu.py::test_every_row_moves_the_frame prints every figure)
MIN_MOVED = {name: 0.2 for name in ROWS}
MIN_MOVED["bg0.25"] = 0.3
MIN_MOVED["max_steps1"] = 0.49
OVER_ALL_PIXELS = ("bg0.25",)
# The Sine model's object is thin: from the default camera, under density_scale 0.37 or max_steps 7, fewer than 2 % of the pixels
# keep alpha > 0.5 (fewer than 1 % under the ramp 0.7 + 0.9 px / W of rays_clip_oracle), which is what the density-only twin asks
# of its scene.  Its twin and hit rays therefore come from a camera of twice the focal length, and its ramp is 1.2 + 0.6 px / W:
# on the oracle alpha > 0.5 then holds on 0.055 .. 0.45 of the pixels without a limit and 0.046 .. 0.34 under the ramp, and the hit
# share at opacity 0.5 is 0.055 under max_steps 7 and 0.126 .. 0.45 under the other reduced rows.
SINE_ZOOM = 2.0
SINE_RAMP = (1.2, 0.6)
SINE_HIT_SHARE = {"max_steps7": 0.04}  # every other reduced row: the 0.1 the Sine rows are held to elsewhere


def zoomed_camera(W, H, zoom):
    """synthetic.default_camera with the focal length multiplied by `zoom`"""
    import synthetic as syn
    cam = syn.default_camera(W, H)
    cam[:2] *= np.float32(zoom)
    return cam


def fields(name, bound=1.0):
    """The nrf_options fields of a row for a model of `bound`"""
    kw = dict(ALL_ROWS[name])
    if isinstance(kw.get("min_near"), dict):
        kw["min_near"] = kw["min_near"][float(bound)]
    return kw


def options(name, bound=1.0):
    """nrf_options: the defaults with the row's fields"""
    o = nh.default_options()
    for k, v in fields(name, bound).items():
        setattr(o, k, v)
    return o


def moved(frame, default, over_all=False):
    """MOVED: the share of the pixels with default alpha > 0 (over_all: of all pixels) whose rgba or depth differs from the
    default-options frame by more than 8 / 255.  frame, default: (rgba [..][4], depth [..]) of the same rays."""
    rgba, depth = np.asarray(frame[0], np.float32).reshape(-1, 4), np.asarray(frame[1], np.float32).reshape(-1)
    rgba0, depth0 = np.asarray(default[0], np.float32).reshape(-1, 4), np.asarray(default[1], np.float32).reshape(-1)
    differs = np.any(np.abs(rgba - rgba0) > THRESHOLD, axis=1) | (np.abs(depth - depth0) > THRESHOLD)
    over = np.ones(len(rgba0), bool) if over_all else rgba0[:, 3] > 0
    return float(np.mean(differs[over])) if over.any() else 0.0


def assert_moved(name, frame, default, what=None):
    """The condition a twin test under a row rests on (no condition for the exact rows: their frames are asserted outright)"""
    if name not in ROWS:
        return None
    share = moved(frame, default, name in OVER_ALL_PIXELS)
    print(f"{what or name}: {name} moves {share:.3f} of the {'pixels' if name in OVER_ALL_PIXELS else 'touched pixels'} (at least {MIN_MOVED[name]})")
    assert share >= MIN_MOVED[name], (what, name, share)
    return share
