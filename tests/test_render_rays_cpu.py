"""nrf_render_rays, the parts that need no GPU: the ray guard (the very function the RAYS kernel instances apply per ray,
exported as the diagnostic nrf_debug_ray_valid), the oracle for arbitrary rays that the GPU tests check frames against
(tests/rays_oracle.py, pinned here against nrfo_render), and the entry point's place in the ABI."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import models
import nerfhip as nh
import oracle_py as op
import rays_forms as rf
import rays_oracle as ro
import render_options as rows
import synthetic as syn

W, H = 64, 48


def _ray_valid():
    fn = nh.load_library().nrf_debug_ray_valid
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]

    def valid(o, d):
        o = np.ascontiguousarray(o, np.float32)
        d = np.ascontiguousarray(d, np.float32)
        return bool(fn(o.ctypes.data_as(C.POINTER(C.c_float)), d.ctypes.data_as(C.POINTER(C.c_float))))
    return valid


def test_ray_guard_rejects_what_the_march_cannot_take():
    valid = _ray_valid()
    o0, d0 = [0.1, -0.2, 0.3], [0.0, 0.6, 0.8]
    assert valid(o0, d0)
    for bad in (np.nan, np.inf, -np.inf):
        for i in range(3):
            o, d = list(o0), list(d0)
            o[i] = bad
            assert not valid(o, d0), ("o", i, bad)
            d[i] = bad
            assert not valid(o0, d), ("d", i, bad)
    assert not valid(o0, [0.0, 0.0, 0.0])
    # |o| just beyond 4096 (MAX_CAMERA_DISTANCE), along an axis and along the diagonal
    assert valid([4096.0, 0.0, 0.0], d0)
    assert not valid([np.nextafter(np.float32(4096.0), np.float32(1e9)), 0.0, 0.0], d0)
    assert not valid([0.0, -4097.0, 0.0], d0)
    s = 4096.0 / np.sqrt(3.0)
    assert valid([0.999 * s] * 3, d0) and not valid([1.001 * s] * 3, d0)
    assert not valid([1e30, 0.0, 0.0], d0)  # (the squared norm overflows)
    # |d|^2 just outside [0.25, 4]
    assert valid([0.0, 0.0, 0.5], [0.5, 0.0, 0.0]) and valid(o0, [0.0, 2.0, 0.0])
    assert not valid(o0, [np.nextafter(np.float32(0.5), np.float32(0.0)), 0.0, 0.0])
    assert not valid(o0, [0.0, np.nextafter(np.float32(2.0), np.float32(3.0)), 0.0])
    assert not valid(o0, [0.0, 0.0, 1e-3]) and not valid(o0, [3.0, 0.0, 0.0])


def test_ray_guard_accepts_axis_aligned_and_generated_rays():
    valid = _ray_valid()
    for i in range(3):
        for s in (1.0, -1.0):
            d = [0.0, 0.0, 0.0]
            d[i] = s
            assert valid([0.3, 0.2, -0.1], d), d  # two zero components: the slab tests' nan branch takes them
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    orc = op.Oracle(desc)
    for az, el in ((30.0, 30.0), (200.0, -15.0), (95.0, 80.0)):
        o, d, _, _ = orc.generate_rays(syn.default_camera(W, H), syn.orbit_pose(az, el), W, H)
        assert all(valid(o[i], d[i]) for i in range(len(o))), (az, el)


MODELS = {"bound1": dict(), "bound4-cascade3": dict(bound=4.0, cascade=3)}
# rows under which few or no samples are composited by construction: max_steps 1 composites one sample per live ray, a min_near
# beyond every far leaves no ray alive
DEAD_ROWS = ("max_steps1", "min_near_beyond_far")


@functools.lru_cache(maxsize=None)
def _model(name):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **MODELS[name])
    return desc, keep, op.Oracle(desc)


# (the default-options cases keep the ids they have always had: the model's name alone)
ASSEMBLED_CASES = [(m, r) for m in MODELS for r in ["default"] + list(rows.ALL_ROWS)]


@pytest.mark.parametrize("model,row", ASSEMBLED_CASES, ids=[m if r == "default" else f"{m}-{r}" for m, r in ASSEMBLED_CASES])
def test_assembled_oracle_reproduces_the_per_ray_render(model, row):
    """nrfo_march(1) -> nrfo_network -> nrfo_composite per ray, numpy near / far, the finish epilogue == nrfo_render(SCHED_PER_RAY),
    bit for bit, on the rays nrfo_generate_rays writes for the camera -- under the default options and under every row of
    tests/render_options.py (density_scale: the checker's own fp32 product)."""
    desc, keep, orc = _model(model)
    cam, pose = syn.default_camera(W, H), syn.orbit_pose(30, 30)
    opts = nh.default_options() if row == "default" else rows.options(row, desc.bound)
    want, wdepth, wst = orc.render(cam, pose, W, H, opts, schedule=op.SCHED_PER_RAY)
    o, d, nr, fr = orc.generate_rays(cam, pose, W, H, opts)
    near, far = ro.near_far([desc.aabb[i] for i in range(6)], o, d, opts.min_near)
    assert np.array_equal(near.view(np.uint32), nr.view(np.uint32)) and np.array_equal(far.view(np.uint32), fr.view(np.uint32))
    rgba, depth, n = ro.render(orc, desc, o, d, opts)
    print(f"{model} {row}: {n} samples")
    assert n == wst.n_samples, (n, wst.n_samples)
    if row not in DEAD_ROWS:
        assert n > 1000, n
    assert np.array_equal(rgba.reshape(H, W, 4).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(depth.reshape(H, W).view(np.uint32), wdepth.view(np.uint32))
    bg = np.float32(opts.bg_color)
    if row in rows.EXACT_ROWS:  # what the GPU tests assert of these rows holds on the oracle
        assert np.all(rgba[:, :3] == bg) and np.all(rgba[:, 3] == 0) and np.all(depth == 0), row
    if row == "min_near_beyond_far":
        assert n == 0 and not np.any(near < far)
        plain = ro.near_far([desc.aabb[i] for i in range(6)], o, d, nh.default_options().min_near)
        assert np.mean(plain[0] < plain[1]) > 0.9 and float(plain[1][plain[0] < plain[1]].max()) < opts.min_near
    if row == "density_scale0":  # the count depends on the march alone: the default frame's rays stop early, these never do
        assert n > _model_default(model)[2].n_samples
    if row == "max_steps1":
        assert 0 < n <= int(np.sum(near < far)) and n >= int(np.sum(rgba[:, 3] > 0))  # at most one sample per live ray


@functools.lru_cache(maxsize=None)
def _model_default(model, w=W, h=H):
    desc, keep, orc = _model(model)
    return orc.render(syn.default_camera(w, h), syn.orbit_pose(30, 30), w, h, nh.default_options(), schedule=op.SCHED_PER_RAY)


def test_the_checker_without_the_multiply_differs():
    """The mutation the parametrised test above must catch: the assembled checker with density_scale left out is NOT the oracle's
    frame under density_scale 0.37 (and is the default frame: the multiply is all that scale does there)."""
    desc, keep, orc = _model("bound1")
    cam, pose = syn.default_camera(W, H), syn.orbit_pose(30, 30)
    opts = rows.options("density_scale0.37")
    want, wdepth, wst = orc.render(cam, pose, W, H, opts, schedule=op.SCHED_PER_RAY)
    o, d, _, _ = orc.generate_rays(cam, pose, W, H, opts)
    rgba, depth, n = ro.render(orc, desc, o, d, opts, apply_density_scale=False)
    differs = np.any(rgba.reshape(H, W, 4).view(np.uint32) != want.view(np.uint32), axis=2)
    print(f"without the multiply {np.mean(differs):.3f} of the pixels differ in their bits, samples {n} against {wst.n_samples}")
    assert np.mean(differs) > 0.3 and n != wst.n_samples
    assert rows.moved((rgba, depth), (want, wdepth)) >= 0.2
    plain = _model_default("bound1")
    assert np.array_equal(rgba.reshape(H, W, 4).view(np.uint32), plain[0].view(np.uint32)) and n == plain[2].n_samples


# every (model, frame) at which tests/test_render_options_gpu.py asserts that a row moved the frame, with the rows it uses there
STAGE_MODELS = {"wide-frequency12": dict(dir_otype="Frequency", n_frequencies=12), "generic-sine": dict(activation="Sine"),
                "generic-F4-w32": dict(n_features_per_level=4, n_neurons=32)}
FORM_ROWS = ["h30", "h64-b1.5-c2", "wide-h30"]
MOVED_SHAPES = ([(m, kw, w, h, list(rows.ROWS), 1.0) for m, kw in MODELS.items() for w, h in ((64, 48), (33, 70))] +
                [(m, kw, 100, 52, rows.REDUCED, 1.0) for m, kw in STAGE_MODELS.items()] +
                [("generic-sine", STAGE_MODELS["generic-sine"], 100, 52, rows.REDUCED, rows.SINE_ZOOM)] +
                [(r, None, rf.RW, rf.RH, rows.REDUCED, 1.0) for r in FORM_ROWS])


@pytest.mark.parametrize("model,kw,w,h,names,zoom", MOVED_SHAPES, ids=[f"{s[0]}-{s[2]}x{s[3]}-zoom{s[5]:g}" for s in MOVED_SHAPES])
def test_every_row_moves_the_frame(model, kw, w, h, names, zoom):
    """What the bit-for-bit twins of the GPU file rest on: a twin cannot see an option both of its sides ignore, so each of them
    also asserts that the row moved its frame -- a condition that has to hold on the oracle first, at every model and frame size
    used there.  rows.moved: the share of the pixels the default frame touches whose rgba or depth moves by more than 8 / 255; at
    least 0.2 (bg0.25: 0.3 of all pixels; max_steps1: 0.49, half of the smallest share measured here, 0.982).  Measured: the weakest row is dt_gamma0 on
    the wide models, 0.32; bg0.25 moves 0.58 .. 0.75 of all pixels."""
    desc, keep, _ = rf.build(model) if kw is None else models.build_model(log2_hashmap_size=12, H=32, **kw)
    orc = op.Oracle(desc)
    cam, pose = rows.zoomed_camera(w, h, zoom), syn.orbit_pose(30, 30)
    default = orc.render(cam, pose, w, h, nh.default_options(), schedule=op.SCHED_PER_RAY)
    assert np.mean(default[0][..., 3] > 0) > 0.2
    for name in names:
        frame = orc.render(cam, pose, w, h, rows.options(name, desc.bound), schedule=op.SCHED_PER_RAY)
        rows.assert_moved(name, frame, default, (model, w, h, zoom))


def test_near_far_restatement_handles_zero_direction_components():
    aabb = [-1.0] * 3 + [1.0] * 3
    o = np.array([[0.2, 0.1, -3.0], [0.2, 1.5, -3.0], [0.0, 0.0, 0.0]], np.float32)
    d = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], np.float32)
    near, far = ro.near_far(aabb, o, d, 0.2)
    assert near[0] == 2.0 and far[0] == 4.0           # through the box along z
    assert near[1] == ro.FLT_MAX and far[1] == ro.FLT_MAX  # beside it
    assert far[2] == 1.0                              # from the centre; 0 * inf = NaN fails every comparison, as in C
    assert near[2] == np.float32(0.2)


def test_render_rays_is_part_of_the_abi():
    assert "nrf_render_rays" in nh.exported_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", str(nh.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert {"nrf_render_rays", "nrf_debug_ray_valid", "nrf_debug_rays_instance"} <= names
    assert nh.load_library().nrf_abi_version() == 7 == nh.NRF_ABI_VERSION
    assert hasattr(nh.NerfHip, "render_rays")
