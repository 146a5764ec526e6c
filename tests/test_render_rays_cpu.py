"""nrf_render_rays, the parts that need no GPU: the ray guard (the very function the RAYS kernel instances apply per ray,
exported as the diagnostic nrf_debug_ray_valid), the oracle for arbitrary rays that the GPU tests check frames against
(tests/rays_oracle.py, pinned here against nrfo_render), and the entry point's place in the ABI."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import models
import nerfhip as nh
import oracle_py as op
import rays_oracle as ro
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


@pytest.mark.parametrize("kw", [dict(), dict(bound=4.0, cascade=3)], ids=["bound1", "bound4-cascade3"])
def test_assembled_oracle_reproduces_the_per_ray_render(kw):
    """nrfo_march(1) -> nrfo_network -> nrfo_composite per ray, numpy near / far, the finish epilogue == nrfo_render(SCHED_PER_RAY),
    bit for bit, on the rays nrfo_generate_rays writes for the camera."""
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **kw)
    orc = op.Oracle(desc)
    cam, pose = syn.default_camera(W, H), syn.orbit_pose(30, 30)
    opts = nh.default_options()
    assert opts.density_scale == 1.0
    want, wdepth, wst = orc.render(cam, pose, W, H, opts, schedule=op.SCHED_PER_RAY)
    o, d, nr, fr = orc.generate_rays(cam, pose, W, H, opts)
    near, far = ro.near_far([desc.aabb[i] for i in range(6)], o, d, opts.min_near)
    assert np.array_equal(near.view(np.uint32), nr.view(np.uint32)) and np.array_equal(far.view(np.uint32), fr.view(np.uint32))
    rgba, depth, n = ro.render(orc, desc, o, d, opts)
    assert n == wst.n_samples and n > 1000, (n, wst.n_samples)
    assert np.array_equal(rgba.reshape(H, W, 4).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(depth.reshape(H, W).view(np.uint32), wdepth.view(np.uint32))


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
