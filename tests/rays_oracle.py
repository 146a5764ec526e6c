"""An oracle for frames from ARBITRARY rays, assembled from committed parts of the CPU oracle -- TEST INFRASTRUCTURE ONLY.

The oracle library renders pinhole views only (nrfo_render).  For caller-supplied rays (nrf_render_rays) the same per-ray
loop is put together here from its stage entry points:

    near / far      a fp32 numpy restatement of kernel_near_far_from_aabb (oracle/nerf_oracle.cpp near_far)
    per iteration   nrfo_march(n_step = 1) -> nrfo_network -> nrfo_composite   (render_rays_independent: a ray marches
                    one sample, evaluates it, composites it, until it dies or max_steps iterations have passed)
    epilogue        get_image_and_depth (oracle/nerf_oracle.cpp `finish`)

On the rays nrfo_generate_rays writes for a camera this is bit-identical to nrfo_render(.., SCHED_PER_RAY) of that camera
(tests/test_render_rays_cpu.py) -- which pins this checker, not the feature.  nrfo_network has no scale argument, so
density_scale is applied here: sigma = float32(density_scale) * sigma, one fp32 product right after the network, skipped when the
scale is 1 (network_one of oracle/nerf_oracle.cpp) -- bit for bit under every row of tests/render_options.py."""
from __future__ import annotations

import numpy as np

import nerfhip as nh

FLT_MAX = np.float32(3.402823466e+38)


def near_far(aabb, rays_o, rays_d, min_near):
    """kernel_near_far_from_aabb (render_utils.h:353-391) in fp32, every operation rounded: (near, far) per ray; a ray that
    misses the box gets FLT_MAX twice.  Zero direction components give infinities / NaN exactly as in the C code."""
    aabb = np.asarray(aabb, np.float32)
    o = np.asarray(rays_o, np.float32).reshape(-1, 3)
    d = np.asarray(rays_d, np.float32).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rd = np.float32(1) / d

        def slab(a):
            lo = (aabb[a] - o[:, a]) * rd[:, a]
            hi = (aabb[a + 3] - o[:, a]) * rd[:, a]
            swap = lo > hi
            return np.where(swap, hi, lo), np.where(swap, lo, hi)

        near, far = slab(0)
        ny, fy = slab(1)
        miss = (near > fy) | (ny > far)
        near = np.where(ny > near, ny, near)
        far = np.where(fy < far, fy, far)
        nz, fz = slab(2)
        miss |= (near > fz) | (nz > far)
        near = np.where(nz > near, nz, near)
        far = np.where(fz < far, fz, far)
        near = np.where(near < np.float32(min_near), np.float32(min_near), near)
    near = np.where(miss, FLT_MAX, near).astype(np.float32)
    far = np.where(miss, FLT_MAX, far).astype(np.float32)
    return near, far


def render(oracle, desc, rays_o, rays_d, opts=None, apply_density_scale=True):
    """rgba [n][4], depth [n], samples (the march-emitted samples = what the per-ray schedule composites) for n rays.
    apply_density_scale=False leaves the multiply out: only for the test that shows the checker notices its absence."""
    opts = opts or nh.default_options()
    assert opts.perturb == 0
    scale = np.float32(opts.density_scale)
    o = np.ascontiguousarray(rays_o, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(rays_d, np.float32).reshape(-1, 3)
    n = len(o)
    near, far = near_far([desc.aabb[i] for i in range(6)], o, d, opts.min_near)
    t = near.copy()                                  # init_step0
    state = np.zeros((n, 5), np.float32)             # weight_sum, depth, r, g, b
    alive = np.flatnonzero(near < far)               # a ray with near >= far never enters the alive list
    n_samples = 0
    for _ in range(int(opts.max_steps)):
        if len(alive) == 0:
            break
        xyz, dirs, deltas = oracle.march(o[alive], d[alive], t[alive], far[alive], 1, opts)
        found = deltas[:, 0, 0] != 0                 # (a march that emitted nothing leaves its row zero: the ray dies in composite)
        sig = np.zeros((len(alive), 1), np.float32)
        rgb = np.zeros((len(alive), 1, 3), np.float32)
        if found.any():
            s, c = oracle.network(xyz[found, 0], d[alive][found])
            if apply_density_scale and opts.density_scale != 1.0:
                s = (scale * np.asarray(s, np.float32)).astype(np.float32)
            sig[found, 0] = s
            rgb[found, 0] = c
        n_samples += int(found.sum())
        t_new, st_new = oracle.composite(sig, rgb, deltas, t[alive], state[alive])
        t[alive] = t_new
        state[alive] = st_new
        alive = alive[t_new >= 0]
    bg = np.float32(opts.bg_color)
    rgba = np.empty((n, 4), np.float32)
    w = (np.float32(1) - state[:, 0]) * bg           # image + (1 - weights_sum) * bg_color, every operation rounded
    rgba[:, 0] = w + state[:, 2]
    rgba[:, 1] = w + state[:, 3]
    rgba[:, 2] = w + state[:, 4]
    rgba[:, 3] = state[:, 0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        span = far - near
        depth = np.where(span > 0, np.maximum(state[:, 1] - near, np.float32(0)) / np.where(span > 0, span, np.float32(1)), np.float32(0))
    return rgba, depth.astype(np.float32), n_samples


# ---- ray sets a pinhole cannot describe (ngp units, row-major pixels)
def orthographic(W, H, azimuth_deg=30.0, elevation_deg=30.0, half_extent=1.2, distance=3.0, centre=(0.0, 0.0, 0.0)):
    """Origins on a plane `distance` in front of `centre`, one shared unit direction: every ray has its own origin."""
    az, el = np.radians(azimuth_deg), np.radians(elevation_deg)
    fwd = -np.array([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)])
    up0 = np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up0)
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    u = ((np.arange(W) + 0.5) / W * 2 - 1) * half_extent
    v = (1 - (np.arange(H) + 0.5) / H * 2) * half_extent * H / W
    o = np.asarray(centre) - distance * fwd + u[None, :, None] * right + v[:, None, None] * up
    d = np.broadcast_to(fwd, o.shape)
    return o.reshape(-1, 3).astype(np.float32), np.ascontiguousarray(d.reshape(-1, 3), np.float32)


def equirectangular(W, H, origin):
    """A full panorama from one point: longitude over the columns, latitude over the rows (unit directions)."""
    lon = ((np.arange(W) + 0.5) / W * 2 - 1) * np.pi
    lat = (0.5 - (np.arange(H) + 0.5) / H) * np.pi
    lon, lat = np.meshgrid(lon, lat)
    d = np.stack([np.cos(lat) * np.cos(lon), np.sin(lat), np.cos(lat) * np.sin(lon)], axis=-1)
    o = np.broadcast_to(np.asarray(origin, np.float64), d.shape)
    return np.ascontiguousarray(o.reshape(-1, 3), np.float32), d.reshape(-1, 3).astype(np.float32)
