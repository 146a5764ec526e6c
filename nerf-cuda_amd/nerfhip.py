"""ctypes binding of include/nerfhip.h (the C ABI of the HIP render path).

Host-side mirror, in Python, of what ngp::NerfRender does above its kernels:
  * `desc_from_config`  -- NerfRender::load_snapshot + reset_network
    (reference src/nerf_render.cu:431-473, 111-184) and the NerfNetwork ctor's
    defaulting (include/nerf-cuda/nerf_network.h:95-135): snapshot dict ->
    nrf_model_desc.
  * `NerfHip`           -- thin object over nrf_create / nrf_load_model /
    nrf_set_resolution / nrf_render ... used by tests, bench.py and smoke().

There is no CPU fallback here: if libnerfhip.so is missing or no gfx950 device
is present, construction raises.  The oracle (oracle/) is never imported from
this module.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "libnerfhip.so"

NRF_ABI_VERSION = 7
GATHER_PEER_COPY, GATHER_RCCL = 0, 1  # nrf_group_set_gather
NRF_MAX_VIEWS = 128
NRF_OK, NRF_E_INVALID, NRF_E_UNSUPPORTED, NRF_E_NODEVICE, NRF_E_HIP, NRF_E_STATE, NRF_E_PARAMS = range(7)

ACT = {"none": 0, "relu": 1, "exponential": 2, "sigmoid": 3, "squareplus": 4, "softplus": 5, "sine": 6}
DIR_SH, DIR_FREQUENCY, DIR_IDENTITY = 0, 1, 2
GRID_HASH, GRID_DENSE, GRID_TILED = 0, 1, 2
INTERP = {"linear": 0, "nearest": 1, "smoothstep": 2}  # T/.../grid.h:1383, common.h string_to_interpolation_type


class ModelDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("grid_type", C.c_uint32),
        ("n_levels", C.c_uint32),
        ("n_features_per_level", C.c_uint32),
        ("log2_hashmap_size", C.c_uint32),
        ("base_resolution", C.c_uint32),
        ("per_level_scale", C.c_float),
        ("interpolation", C.c_uint32),
        ("n_neurons", C.c_uint32),
        ("density_hidden_layers", C.c_uint32),
        ("density_activation", C.c_uint32),
        ("density_output_activation", C.c_uint32),
        ("density_n_output", C.c_uint32),
        ("sigma_activation", C.c_uint32),
        ("rgb_hidden_layers", C.c_uint32),
        ("rgb_activation", C.c_uint32),
        ("rgb_output_activation", C.c_uint32),
        ("dir_encoding", C.c_uint32),
        ("sh_degree", C.c_uint32),
        ("n_frequencies", C.c_uint32),
        ("aabb", C.c_float * 6),
        ("bound", C.c_float),
        ("scale", C.c_float),
        ("cascade", C.c_uint32),
        ("density_grid_size", C.c_uint32),
        ("mean_density", C.c_float),
        ("params", C.POINTER(C.c_float)),
        ("n_params", C.c_uint64),
        ("density_grid", C.POINTER(C.c_float)),
        ("n_density_grid", C.c_uint64),
        ("gather_copy_budget_mb", C.c_uint32),
    ]


class LevelTable(C.Structure):
    _fields_ = [
        ("n_levels", C.c_uint32),
        ("offset", C.c_uint32 * 17),
        ("resolution", C.c_uint32 * 16),
        ("scale", C.c_float * 16),
    ]


class Options(C.Structure):
    _fields_ = [
        ("bg_color", C.c_float),
        ("min_near", C.c_float),
        ("dt_gamma", C.c_float),
        ("max_steps", C.c_int32),
        ("density_scale", C.c_float),
        ("perturb", C.c_int32),
        ("shard_index", C.c_int32),
        ("shard_count", C.c_int32),
        ("fast_interp", C.c_int32),
        ("tile_major", C.c_int32),
    ]


class Frame(C.Structure):
    _fields_ = [
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("n_tiles", C.c_int32),
        ("rgba", C.c_void_p),
        ("depth", C.c_void_p),
        ("tile_major", C.c_int32),
        ("n_views", C.c_int32),
        ("view_stride_px", C.c_int64),
    ]


class HostFrame(C.Structure):
    """nrf_host_frame: 8-bit planes in pinned host memory owned by the context (nrf_submit_host_u8)."""
    _fields_ = [
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("n_views", C.c_int32),
        ("rgb", C.c_void_p),
        ("depth", C.c_void_p),
        ("view_stride_px", C.c_int64),
        ("render_ms", C.c_float),
        ("copied_bytes", C.c_uint64),
    ]


class UpscaleTemporal(C.Structure):
    """nrf_upscale_temporal: one call of the temporal upscaler (nrf_rb_upscale_temporal)."""
    _fields_ = [
        ("motion", C.c_void_p),
        ("jitter", C.c_float * 2),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class Motion(C.Structure):
    """nrf_motion: the planes of a NRF_RAYS_DEPTH_T ray frame, its rays and the two cameras (nrf_motion_vectors)."""
    _fields_ = [
        ("rays_o", C.c_void_p),
        ("rays_d", C.c_void_p),
        ("rgba", C.c_void_p),
        ("depth_t", C.c_void_p),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("out_width", C.c_int32),
        ("out_height", C.c_int32),
        ("min_alpha", C.c_float),
        ("cam", C.c_float * 4),
        ("pose", C.c_float * 16),
        ("prev_cam", C.c_float * 4),
        ("prev_pose", C.c_float * 16),
        ("reserved", C.c_uint32),
    ]


NRF_UPSCALE_T_RESET, NRF_UPSCALE_T_RECTIFY = 1, 2
NRF_HOST_RGB_ONLY = 1
NRF_RAYS_DEPTH_T = 1  # nrf_rays.flags: the depth plane holds the accumulated sum of w * t, not its normalised form
NRF_RAYS_DENSITY_ONLY = 4  # nrf_rays.flags: the density network alone -- alpha and depth as without it, rgb = (1 - alpha) * background


class Rays(C.Structure):
    """nrf_rays: the rays of nrf_render_rays_clipped with their per-ray limits of t and background (device pointers; 0 = none)."""
    _fields_ = [
        ("rays_o", C.c_void_p),
        ("rays_d", C.c_void_p),
        ("rays_per_view", C.c_uint64),
        ("t_min", C.c_void_p),
        ("t_max", C.c_void_p),
        ("background", C.c_void_p),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class Lattice(C.Structure):
    """nrf_lattice: point (i, j, k) of dims = (nx, ny, nz) lies at origin + (i, j, k) * cell and has the index (i * ny + j) * nz + k."""
    _fields_ = [
        ("origin", C.c_float * 3),
        ("cell", C.c_float * 3),
        ("dims", C.c_uint32 * 3),
        ("reserved", C.c_uint32),
    ]

    @classmethod
    def make(cls, origin, cell, dims):
        return cls((C.c_float * 3)(*[float(v) for v in origin]), (C.c_float * 3)(*[float(v) for v in cell]),
                   (C.c_uint32 * 3)(*[int(v) for v in dims]), 0)

    @property
    def n_points(self):
        return int(self.dims[0]) * int(self.dims[1]) * int(self.dims[2])


class Mesh(C.Structure):
    """nrf_mesh: device pointers owned by the context, valid until the next extract_mesh or close."""
    _fields_ = [
        ("n_vertices", C.c_uint64),
        ("n_triangles", C.c_uint64),
        ("vertices", C.c_void_p),   # float [n_vertices][3]
        ("triangles", C.c_void_p),  # uint32 [n_triangles][3]
        ("sigma", C.c_void_p),      # float [nx][ny][nz]
    ]


class MeshAttr(C.Structure):
    """nrf_mesh_attr: device pointers owned by the context, valid until the next extract_mesh, mesh_attributes or close."""
    _fields_ = [
        ("n_vertices", C.c_uint64),
        ("normals", C.c_void_p),  # float4 [n_vertices] = (n_x, n_y, n_z, sigma)
        ("colors", C.c_void_p),   # float4 [n_vertices] = (r, g, b, |g|)
    ]


class MeshParts(C.Structure):
    """nrf_mesh_parts: device pointers owned by the context, valid until the next extract_mesh, filter_mesh, mesh_components or close."""
    _fields_ = [
        ("n_components", C.c_uint64),
        ("labels", C.c_void_p),      # uint32 [n_vertices]
        ("components", C.c_void_p),  # uint32 [n_components][3] = (label, n_vertices, n_triangles), ascending label
        ("n_rounds", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


NRF_MESH_KEEP_LARGEST = 1


class MeshRefine(C.Structure):
    """nrf_mesh_refine: device pointers owned by the context, valid until the next extract_mesh, filter_mesh, refine_mesh or close."""
    _fields_ = [
        ("n_vertices", C.c_uint64),
        ("n_unbracketed", C.c_uint64),  # vertices left as they were
        ("vertices", C.c_void_p),       # float [n_vertices][3]: the mesh's vertex buffer, refined in place
        ("edges", C.c_void_p),          # uint32 [n_vertices] = (p << 3) | m
        ("brackets", C.c_void_p),       # float4 [n_vertices] = (lo, hi, s_lo, s_hi)
        ("n_steps", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class MeshSimplify(C.Structure):
    """nrf_mesh_simplify: device pointers owned by the context, valid until the next extract_mesh, filter_mesh, simplify_mesh or close."""
    _fields_ = [
        ("n_vertices", C.c_uint64),
        ("n_triangles", C.c_uint64),
        ("n_vertices_before", C.c_uint64),
        ("n_triangles_before", C.c_uint64),
        ("vertices", C.c_void_p),    # float [n_vertices][3]: the context's mesh
        ("triangles", C.c_void_p),   # uint32 [n_triangles][3]
        ("edges", C.c_void_p),       # uint32 [n_vertices]: the kept vertices' edge words
        ("sources", C.c_void_p),     # uint32 [n_vertices]: the old id of every kept vertex, ascending
        ("vertex_map", C.c_void_p),  # uint32 [n_vertices_before]: the new id of every old vertex's representative, or 0xffffffff
        ("factor", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class MeshTexture(C.Structure):
    """nrf_mesh_texture: device pointers owned by the context, valid until the next extract_mesh, filter_mesh, refine_mesh,
    simplify_mesh, bake_mesh_texture or close."""
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("res", C.c_uint32),
        ("cols", C.c_uint32),
        ("n_triangles", C.c_uint64),
        ("n_refused", C.c_uint64),   # owned texels the guard zeroed
        ("texels", C.c_void_p),      # float4 [height][width] = (r, g, b, sigma)
        ("rgba8", C.c_void_p),       # uint32 [height][width]
        ("uvs", C.c_void_p),         # float [n_triangles][3][2]
    ]


class Stats(C.Structure):
    _fields_ = [
        ("n_rays", C.c_uint64),
        ("n_samples", C.c_uint64),
        ("n_rounds", C.c_uint64),
        ("n_network_evals", C.c_uint64),
        ("render_ms", C.c_float),
        ("n_composited", C.c_uint64),
        ("shader_clock_mhz", C.c_float),
        ("gather_addresses_per_sample", C.c_uint32),
        ("grid_device_bytes", C.c_uint64),
    ]


def default_options() -> Options:
    """Private member defaults of NerfRender (include/nerf-cuda/nerf_render.h:55-78)."""
    return Options(1.0, 0.2, 1.0 / 128.0, 1024, 1.0, 0, 0, 1, 0)


class NerfHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"nerfhip error {code}: {msg}")
        self.code = code


# --------------------------------------------------------------------------
# library loading
# --------------------------------------------------------------------------
_lib = None

_SIGS = {
    "nrf_last_error": (C.c_char_p, []),
    "nrf_abi_version": (C.c_int, []),
    "nrf_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "nrf_destroy": (C.c_int, [C.c_void_p]),
    "nrf_default_options": (None, [C.POINTER(Options)]),
    "nrf_level_table_compute": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(LevelTable)]),
    "nrf_expected_n_params": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(C.c_uint64)]),
    "nrf_default_per_level_scale": (C.c_int, [C.c_float, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "nrf_load_model": (C.c_int, [C.c_void_p, C.POINTER(ModelDesc)]),
    "nrf_set_resolution": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "nrf_generate_density_grid": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_float)]),
    "nrf_read_density_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_float)]),
    "nrf_set_options": (C.c_int, [C.c_void_p, C.POINTER(Options)]),
    "nrf_render": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.POINTER(Frame)]),
    "nrf_set_max_views": (C.c_int, [C.c_void_p, C.c_int]),
    "nrf_render_views": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p,
                                   C.POINTER(Frame)]),
    "nrf_render_batch": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p,
                                   C.POINTER(Frame)]),
    "nrf_render_rays": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(Frame)]),
    "nrf_render_rays_clipped": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Rays), C.c_void_p, C.POINTER(Frame)]),
    "nrf_ray_hits": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Rays), C.c_float, C.c_void_p, C.POINTER(Frame)]),
    "nrf_read_view_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "nrf_read_view_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "nrf_bind_output": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_bind_output_rgbd8": (C.c_int, [C.c_void_p, C.c_void_p]),
    "nrf_bind_output_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_submit_host_u8": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]),
    "nrf_wait_host_u8": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(HostFrame)]),
    "nrf_render_host_u8": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(HostFrame)]),
    "nrf_quantize_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_untile_views_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_group_submit_host_u8": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int,
                                           C.POINTER(C.c_int)]),
    "nrf_group_wait_host_u8": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(HostFrame)]),
    "nrf_group_render_host_u8": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int,
                                           C.POINTER(HostFrame)]),
    "nrf_render_async": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(Frame)]),
    "nrf_sync": (C.c_int, [C.c_void_p]),
    "nrf_generate_rays_host": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "nrf_read_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_read_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_read_shard_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_untile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nrf_quantize_rgbd8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "nrf_group_create": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "nrf_group_destroy": (C.c_int, [C.c_void_p]),
    "nrf_group_size": (C.c_int, [C.c_void_p]),
    "nrf_group_member": (C.c_void_p, [C.c_void_p, C.c_int]),
    "nrf_group_load_model": (C.c_int, [C.c_void_p, C.POINTER(ModelDesc)]),
    "nrf_group_set_options": (C.c_int, [C.c_void_p, C.POINTER(Options)]),
    "nrf_group_set_resolution": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "nrf_group_render_views": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(Frame)]),
    "nrf_group_read_view_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "nrf_group_read_view_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "nrf_group_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "nrf_group_set_gather": (C.c_int, [C.c_void_p, C.c_int]),
    "nrf_group_get_gather": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nrf_untile_views": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nrf_tiles_per_shard": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "nrf_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "nrf_rb_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "nrf_rb_destroy": (C.c_int, [C.c_void_p]),
    "nrf_rb_resize": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "nrf_rb_reset_accumulation": (C.c_int, [C.c_void_p]),
    "nrf_rb_spp": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "nrf_rb_set_color_space": (C.c_int, [C.c_void_p, C.c_int]),
    "nrf_rb_set_tonemap_curve": (C.c_int, [C.c_void_p, C.c_int]),
    "nrf_rb_buffers": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_void_p)]),
    "nrf_rb_clear_frame": (C.c_int, [C.c_void_p, C.c_void_p]),
    "nrf_rb_accumulate": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p]),
    "nrf_rb_tonemap": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    "nrf_rb_present": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p]),
    "nrf_rb_overlay_depth": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_float,
                                       C.POINTER(C.c_float), C.c_void_p]),
    "nrf_rb_host_to_accumulate_buffer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "nrf_rb_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_rb_srgb8_table": (C.c_int, [C.POINTER(C.c_float)]),
    "nrf_rb_overlay_image": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_float), C.c_void_p]),
    "nrf_rb_overlay_false_color": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                             C.c_int, C.c_void_p]),
    "nrf_rb_error_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_rb_enable_upscale": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "nrf_rb_disable_upscale": (C.c_int, [C.c_void_p]),
    "nrf_rb_set_upscale_sharpening": (C.c_int, [C.c_void_p, C.c_float]),
    "nrf_rb_resolutions": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nrf_rb_upscale": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_rb_upscaled": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "nrf_rb_read_upscaled": (C.c_int, [C.c_void_p, C.c_void_p]),
    "nrf_rb_upscale_jitter": (C.c_int, [C.c_uint32, C.POINTER(C.c_float)]),
    "nrf_rb_set_upscale_history": (C.c_int, [C.c_void_p, C.c_float]),
    "nrf_rb_upscale_temporal": (C.c_int, [C.c_void_p, C.POINTER(UpscaleTemporal), C.c_void_p, C.c_void_p]),
    "nrf_rb_upscale_history": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]),
    "nrf_rb_read_upscale_history": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_motion_vectors": (C.c_int, [C.c_void_p, C.POINTER(Motion), C.c_void_p, C.c_void_p]),
    "nrf_encode_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "nrf_encode_dir": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "nrf_mlp_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "nrf_mlp_forward_repeat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "nrf_network": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_density": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "nrf_density_gradient": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]),
    "nrf_hit_gradients": (C.c_int, [C.c_void_p, C.POINTER(Frame), C.POINTER(Rays), C.c_float, C.c_float, C.c_float, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "nrf_density_lattice": (C.c_int, [C.c_void_p, C.POINTER(Lattice), C.c_void_p, C.c_void_p]),
    "nrf_extract_mesh": (C.c_int, [C.c_void_p, C.POINTER(Lattice), C.c_float, C.c_void_p, C.c_void_p, C.POINTER(Mesh)]),
    "nrf_read_mesh": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "nrf_point_attributes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_mesh_attributes": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.POINTER(MeshAttr)]),
    "nrf_read_mesh_attributes": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "nrf_mesh_components": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(MeshParts)]),
    "nrf_read_mesh_components": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "nrf_filter_mesh": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(Mesh)]),
    "nrf_refine_mesh": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(MeshRefine)]),
    "nrf_read_mesh_refinement": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "nrf_simplify_mesh": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(MeshSimplify)]),
    "nrf_read_mesh_simplification": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "nrf_mesh_texture_size": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "nrf_bake_mesh_texture": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(MeshTexture)]),
    "nrf_read_mesh_texture": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "nrf_generate_rays": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_march": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrf_composite": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                C.c_void_p, C.c_void_p]),
}


def exported_symbols():
    """Names include/nerfhip.h declares (checked against the .so by the CPU tests)."""
    return sorted(_SIGS)


def load_library(path: os.PathLike | None = None):
    """dlopen libnerfhip.so and attach signatures.  Fails loudly when missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise FileNotFoundError(
            f"{p} not found: build it with `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(str(p))
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError = symbol missing from the .so
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _check(rc: int):
    if rc != NRF_OK:
        raise NerfHipError(rc, load_library().nrf_last_error().decode("utf-8", "replace"))


# --------------------------------------------------------------------------
# snapshot dict -> nrf_model_desc  (load_snapshot + reset_network + NerfNetwork ctor)
# --------------------------------------------------------------------------
def _act(name, default):
    s = (name if name is not None else default).lower()
    if s not in ACT:
        raise ValueError(f"Invalid activation name: {name}")  # T/src/network.cu:41-60
    return ACT[s]


def default_per_level_scale(bound: float, base_resolution: int, n_levels: int) -> float:
    """fp32 exp(log(2048*bound/base)/(L-1)), reference src/nerf_render.cu:158-165.
    Evaluated by the C library so that libm's expf/logf are used."""
    out = C.c_float()
    _check(load_library().nrf_default_per_level_scale(C.c_float(bound), base_resolution, n_levels, C.byref(out)))
    return float(out.value)


def srgb8_table():
    """float32 [256]: srgb_to_linear(b / 255) as the image overlay reads a Byte texel's channels (nrf_rb_srgb8_table; host only)."""
    t = (C.c_float * 256)()
    _check(load_library().nrf_rb_srgb8_table(t))
    return np.frombuffer(t, np.float32).copy()


def upscale_jitter(k: int):
    """(jx, jy) of frame k of the temporal upscaler's jitter sequence (nrf_rb_upscale_jitter): Halton bases 2 and 3, in [-0.5, 0.5)."""
    j = (C.c_float * 2)()
    _check(load_library().nrf_rb_upscale_jitter(k, j))
    return float(j[0]), float(j[1])


# --------------------------------------------------------------------------
# instant-ngp snapshots (the reference itself only reads its own array form, nerf_render.cu:441-453)
# --------------------------------------------------------------------------
# Layout, from instant-ngp's public Testbed::save_snapshot / load_snapshot and NerfNetwork (the reference's
# nerf_network.h is derived from the latter, so the parameter order -- density MLP | rgb MLP | hash grid -- and the
# row-major [out][in] matrices are the same):
#   snapshot.params_binary      raw little-endian blob of snapshot.params_type ("__half" | "float"), snapshot.n_params values
#   snapshot.density_grid_size  128
#   snapshot.density_grid_binary  (K+1) * 128^3 values ("__half", or "float" in the first format revision -- told apart
#                               by the blob's size), K = log2(aabb_scale); value of cell (x, y, z) of cascade c at
#                               c * 128^3 + morton3D(x, y, z); cascade c is the cube of side 2^c around (0.5, 0.5, 0.5)
#   snapshot.nerf.aabb_scale    (also snapshot.nerf.dataset.aabb_scale); snapshot.nerf.dataset.scale / .offset = 0.33 / 0.5
#   snapshot.aabb               {"min": [3], "max": [3]} in instant-ngp's unit-cube coordinates
# Mapping onto the reference's conventions (torch-ngp's, which it restates): coordinates x_ref = x_ngp - 0.5,
# bound = aabb_scale / 2 (so x_ref / (2 bound) + 0.5 is instant-ngp's position inside its aabb); the reference's cascade k
# is the cube +-min(2^k, bound), i.e. instant-ngp's cascade k + 1 (cascade 0 for aabb_scale 1), each cell taking the
# maximum of its own value and of its eight children in the next finer instant-ngp cascade (instant-ngp's own bitfield
# is max-pooled that way); mean_density = mean(max(v, 0)) over instant-ngp's cascade 0, as instant-ngp computes it;
# per_level_scale, when the file leaves it out, is instant-ngp's exp(log(2048 aabb_scale / N_min) / (L - 1)); and
# the colour activation instant-ngp applies outside its network (logistic) becomes rgb_network.output_activation.
def morton3d(x, y, z):
    """x | y << 1 | z << 2 bit-interleaved (instant-ngp's morton3D; the reference carries the same helper, render_utils.h:157-170)."""
    def expand(v):
        v = (v * 0x00010001) & 0xFF0000FF
        v = (v * 0x00000101) & 0x0F00F00F
        v = (v * 0x00000011) & 0xC30C30C3
        v = (v * 0x00000005) & 0x49249249
        return v
    x, y, z = (np.asarray(a, np.uint64) for a in (x, y, z))
    return (expand(x) | (expand(y) << np.uint64(1)) | (expand(z) << np.uint64(2))).astype(np.uint32)


def blob_bytes(value, what: str) -> bytes:
    """A binary value of a snapshot as bytes.  tcnn writes its parameters with `gpu_memory_to_json_binary` (a nlohmann
    binary_t: msgpack `bin`) and READS either that or, from a text JSON, the object `{"bytes": [..], "subtype": ..}`
    (T/include/tiny-cuda-nn/gpu_memory_json.h:37-72): both are accepted here."""
    if isinstance(value, (bytes, bytearray, memoryview)):
        return bytes(value)
    if isinstance(value, dict) and "bytes" in value:
        return bytes(bytearray(int(v) & 0xff for v in value["bytes"]))
    raise RuntimeError(f"{what}: Invalid json type: must be either binary or object")  # gpu_memory_json.h:70


def is_ngp_snapshot(config: dict) -> bool:
    snap = config.get("snapshot", {})
    return isinstance(snap, dict) and ("nerf" in snap or isinstance(snap.get("aabb"), dict))


def ngp_snapshot_to_reference(config: dict) -> dict:
    """An instant-ngp snapshot dict -> the same model as a snapshot dict in the reference's own format."""
    snap = config["snapshot"]
    nerf = snap.get("nerf", {})
    dataset = nerf.get("dataset", {})
    aabb_scale = int(nerf.get("aabb_scale", dataset.get("aabb_scale", 1)))
    if aabb_scale < 1 or aabb_scale & (aabb_scale - 1):
        raise RuntimeError("instant-ngp snapshot: aabb_scale must be a power of two")
    offset = dataset.get("offset", [0.5, 0.5, 0.5])
    if any(abs(float(v) - 0.5) > 1e-6 for v in offset):
        raise NotImplementedError("instant-ngp snapshot: dataset.offset other than 0.5 has no counterpart in the reference")
    H = int(snap.get("density_grid_size", 128))
    if H & (H - 1):
        raise RuntimeError("instant-ngp snapshot: density_grid_size must be a power of two (Morton order)")
    n_ngp = aabb_scale.bit_length()  # K + 1 cascades
    blob = blob_bytes(snap["density_grid_binary"], "snapshot.density_grid_binary")
    cells = n_ngp * H ** 3
    kind = snap.get("density_grid_type")
    if kind is None:
        kind = "float" if len(blob) == 4 * cells else "__half"
    grid = np.frombuffer(blob, np.float32 if kind == "float" else np.float16).astype(np.float32)
    if grid.size < cells:
        raise RuntimeError("Incompatible number of grid cascades.")
    grid = grid[:cells].reshape(n_ngp, H ** 3)
    ax = np.arange(H, dtype=np.uint32)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    m = morton3d(X, Y, Z).reshape(-1)
    xmajor = grid[:, m].reshape(n_ngp, H, H, H)  # [cascade][x][y][z]
    bound = aabb_scale / 2.0
    C = 1 if aabb_scale == 1 else n_ngp - 1
    out = np.empty((C, H, H, H), np.float32)
    for k in range(C):
        c = 0 if aabb_scale == 1 else k + 1
        own = xmajor[c].copy()
        if c > 0:  # the inner half of cascade c is covered twice as finely by cascade c - 1
            fine = xmajor[c - 1].reshape(H // 2, 2, H // 2, 2, H // 2, 2).max(axis=(1, 3, 5))
            q = H // 4
            inner = own[q:q + H // 2, q:q + H // 2, q:q + H // 2]
            np.maximum(inner, fine, out=inner)
        out[k] = own
    lo, hi = snap.get("aabb", {}).get("min"), snap.get("aabb", {}).get("max")
    if lo is None or hi is None:
        lo, hi = [0.5 - bound] * 3, [0.5 + bound] * 3
    ref = {k: (dict(v) if isinstance(v, dict) else v) for k, v in config.items() if k != "snapshot"}
    enc = ref.setdefault("encoding", {})
    if not float(enc.get("per_level_scale", 0.0)) > 0.0 and int(enc.get("n_levels", 16)) > 1:
        base = int(enc.get("base_resolution", 0)) or (1 << (int(enc.get("log2_hashmap_size", 15)) // 3))
        enc["per_level_scale"] = default_per_level_scale(float(aabb_scale), base, int(enc.get("n_levels", 16)))
    rgb = ref.setdefault("rgb_network", {})
    if str(rgb.get("output_activation", "None")).lower() == "none":
        rgb["output_activation"] = "Sigmoid" if str(nerf.get("rgb_activation", "Logistic")).lower() in ("logistic", "sigmoid") else "None"
    new = {"aabb": [float(v) - 0.5 for v in lo] + [float(v) - 0.5 for v in hi], "bound": float(bound),
           "scale": float(dataset.get("scale", 0.33)), "cascade": int(C), "density_grid_size": H,
           "mean_density": float(np.maximum(xmajor[0], 0.0).mean(dtype=np.float64)),
           "density_grid_binary": out.reshape(-1).tobytes(), "density_grid_type": "float",
           "params_binary": blob_bytes(snap["params_binary"], "snapshot.params_binary"), "params_type": snap.get("params_type", "__half")}
    # tcnn's Trainer::serialize writes `n_params` beside the blob (T/include/tiny-cuda-nn/trainer.h:267-279: sizeof(PARAMS_T) *
    # n_params bytes of the inference parameters, PARAMS_T = __half for a FullyFusedMLP model); a file whose two disagree is corrupt
    if "n_params" in snap:
        width = 4 if new["params_type"] == "float" else 2
        if int(snap["n_params"]) * width != len(new["params_binary"]):
            raise RuntimeError(f"snapshot.params_binary holds {len(new['params_binary']) // width} values, snapshot.n_params says {int(snap['n_params'])}")
    ref["snapshot"] = new
    return ref


def desc_from_config(config: dict, params: np.ndarray | None = None, density_grid: np.ndarray | None = None):
    """Build a nrf_model_desc from a snapshot dict in the reference's format
     -- or in instant-ngp's, which is converted first.  Returns (desc, keepalive)."""
    if "snapshot" not in config:
        raise RuntimeError("File does not contain a snapshot.")  # nerf_render.cu:434-436
    if is_ngp_snapshot(config):
        config = ngp_snapshot_to_reference(config)
    snap = config["snapshot"]
    enc = dict(config.get("encoding", {}))
    net = dict(config.get("network", {}))
    rgb = dict(config.get("rgb_network", {}))
    dire = dict(config.get("dir_encoding", {}))

    d = ModelDesc()
    d.abi_version = NRF_ABI_VERSION
    # snapshot block, nerf_render.cu:441-453 with member defaults nerf_render.h:55-67
    aabb = [float(v) for v in snap["aabb"]]
    d.aabb = (C.c_float * 6)(*aabb)
    d.bound = float(snap.get("bound", 1))
    d.scale = float(snap.get("scale", 0.33))
    d.cascade = int(snap.get("cascade", 1))
    d.density_grid_size = int(snap.get("density_grid_size", 128))
    d.mean_density = float(snap.get("mean_density", 1e-4))

    # encoding block, nerf_render.cu:125-165 and grid.h:1365-1386
    otype = enc.get("otype", "OneBlob").lower()
    if "grid" not in otype:
        raise NotImplementedError(f"position encoding '{otype}' is outside the hot path (hash grid only)")
    default_type = "tiled" if otype == "tiledgrid" else ("dense" if otype == "densegrid" else "hash")
    d.grid_type = {"hash": GRID_HASH, "dense": GRID_DENSE, "tiled": GRID_TILED}[enc.get("type", default_type).lower()]
    F = int(enc.get("n_features_per_level", 2))
    d.n_features_per_level = F
    if enc.get("n_features", 0) and enc["n_features"] > 0:
        if "n_levels" in enc:
            raise RuntimeError("GridEncoding: may not specify n_features and n_levels simultaneously")
        d.n_levels = int(enc["n_features"]) // F
    else:
        d.n_levels = int(enc.get("n_levels", 16))
    d.log2_hashmap_size = int(enc.get("log2_hashmap_size", 15))  # the reference's default, nerf_render.cu:144-145
    base = int(enc.get("base_resolution", 0))
    if not base:
        base = 1 << (d.log2_hashmap_size // 3)
    d.base_resolution = base
    pls = float(enc.get("per_level_scale", 0.0))
    if pls <= 0.0 and d.n_levels > 1:
        pls = default_per_level_scale(d.bound, base, d.n_levels)
    if pls <= 0.0:
        pls = 2.0
    d.per_level_scale = pls
    interp = enc.get("interpolation", "Linear").lower()
    if interp not in INTERP:
        raise RuntimeError(f"Invalid interpolation type: {interp}")
    d.interpolation = INTERP[interp]
    if F not in (1, 2, 4, 8):
        raise RuntimeError("GridEncoding: n_features_per_level must be 1, 2, 4, or 8.")  # grid.h:1403-1411

    # network blocks, T/src/network.cu:127-143 + nerf_network.h:117-135
    def mlp(cfg):
        ot = cfg.get("otype", "FullyFusedMLP").lower()
        if ot not in ("fullyfusedmlp", "megakernelmlp", "mlp", "cutlassmlp"):
            raise RuntimeError(f"Invalid network type: {ot}")
        return int(cfg.get("n_neurons", 128)), int(cfg.get("n_hidden_layers", 5)), \
            _act(cfg.get("activation"), "ReLU"), _act(cfg.get("output_activation"), "None")

    n1, h1, a1, o1 = mlp(net)
    n2, h2, a2, o2 = mlp(rgb)
    if n1 != n2:
        raise NotImplementedError("density and rgb networks must share n_neurons")
    d.n_neurons = n1
    d.density_hidden_layers, d.density_activation, d.density_output_activation = h1, a1, o1
    d.density_n_output = int(net.get("n_output_dims", 16))
    d.sigma_activation = _act(net.get("sigma_activation"), "Exponential")
    d.rgb_hidden_layers, d.rgb_activation, d.rgb_output_activation = h2, a2, o2

    # dir_encoding: Composite{nested[0] on 3 dims, Identity on the remaining 0 dims (dropped)}
    # T/include/tiny-cuda-nn/encodings/composite.h:139-216
    node = dire
    if node.get("otype", "Composite").lower() == "composite":
        # a nested encoding without n_dims_to_encode takes the remaining dims; with all 3
        # consumed by the first, the rest encode 0 dims and are dropped (composite.h:182-185)
        covering = [n for n in node.get("nested", []) if int(n.get("n_dims_to_encode", 0)) == 3]
        if not covering and len(node.get("nested", [])) == 1 and "n_dims_to_encode" not in node["nested"][0]:
            covering = [node["nested"][0]]
        if not covering:
            raise NotImplementedError("dir_encoding must encode all 3 direction dims with one nested encoding")
        node = covering[0]
    ot = node.get("otype", "").lower()
    if ot == "sphericalharmonics":
        d.dir_encoding, d.sh_degree = DIR_SH, int(node.get("degree", 4))
    elif ot == "frequency":
        d.dir_encoding, d.n_frequencies = DIR_FREQUENCY, int(node.get("n_frequencies", 12))
    elif ot == "identity":
        d.dir_encoding = DIR_IDENTITY
    else:
        raise NotImplementedError(f"dir encoding '{ot}' is outside the hot path")

    def numbers(key):
        """`key` as an array of numbers (the reference's format) or `key_binary` + `key_type` (instant-ngp's)."""
        if key in snap:
            return np.asarray(snap[key], dtype=np.float32)
        blob = blob_bytes(snap[key + "_binary"], f"snapshot.{key}_binary")
        kind = snap.get(key + "_type", "__half")
        if kind not in ("__half", "half", "float"):
            raise RuntimeError(f"snapshot.{key}_type: unknown element type '{kind}'")
        return np.frombuffer(blob, np.float32 if kind == "float" else np.float16).astype(np.float32)

    p = np.ascontiguousarray(params if params is not None else numbers("params"), dtype=np.float32)
    d.params = p.ctypes.data_as(C.POINTER(C.c_float))
    d.n_params = p.size
    if density_grid is None and "density_grid" not in snap and "density_grid_binary" not in snap:
        # no grid in the snapshot: NerfRender::generate_density_grid (nrf_generate_density_grid) makes one from the network
        d.density_grid = None
        d.n_density_grid = 0
        return d, (p, None)
    g = np.ascontiguousarray(density_grid if density_grid is not None else numbers("density_grid"), dtype=np.float32)
    d.density_grid = g.ctypes.data_as(C.POINTER(C.c_float))
    d.n_density_grid = g.size
    return d, (p, g)


def level_table(desc: ModelDesc) -> LevelTable:
    t = LevelTable()
    _check(load_library().nrf_level_table_compute(C.byref(desc), C.byref(t)))
    return t


def expected_n_params(desc: ModelDesc) -> int:
    n = C.c_uint64()
    _check(load_library().nrf_expected_n_params(C.byref(desc), C.byref(n)))
    return int(n.value)


def tiles_per_shard(width: int, height: int, shard_count: int) -> int:
    n = C.c_int()
    _check(load_library().nrf_tiles_per_shard(width, height, shard_count, C.byref(n)))
    return int(n.value)


def mesh_texture_size(n_triangles: int, res: int, width: int) -> int:
    """nrf_mesh_texture_size: the height of the atlas bake_mesh_texture makes of n_triangles at (res, width); host only"""
    h = C.c_uint32()
    _check(load_library().nrf_mesh_texture_size(C.c_uint64(int(n_triangles)), C.c_uint32(int(res)), C.c_uint32(int(width)), C.byref(h)))
    return int(h.value)


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _host_frame_arrays(f: HostFrame, copy: bool):
    """numpy views (or copies) of a HostFrame's pinned planes: rgb u8 [n][H][W][3], depth u8 [n][H][W] (or None)."""
    n, h, w, stride = f.n_views, f.height, f.width, int(f.view_stride_px)
    rgb = np.ctypeslib.as_array(C.cast(f.rgb, C.POINTER(C.c_uint8)), shape=(n, stride * 3))[:, :h * w * 3].reshape(n, h, w, 3)
    depth = None
    if f.depth:
        depth = np.ctypeslib.as_array(C.cast(f.depth, C.POINTER(C.c_uint8)), shape=(n, stride))[:, :h * w].reshape(n, h, w)
    if copy:
        rgb = rgb.copy()
        depth = None if depth is None else depth.copy()
    return rgb, depth


def _views(cams, poses):
    cams = np.ascontiguousarray(cams, dtype=np.float32).reshape(-1, 4)
    poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
    if len(cams) != len(poses):
        raise ValueError("cams and poses must have the same length")
    return cams, poses


class NerfHip:
    """One context on one device (nrf_context)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        _check(self.lib.nrf_create(device, C.byref(h)))
        self.h = h
        self.width = self.height = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.nrf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_model(self, desc: ModelDesc):
        _check(self.lib.nrf_load_model(self.h, C.byref(desc)))

    def set_resolution(self, width: int, height: int):
        _check(self.lib.nrf_set_resolution(self.h, width, height))
        self.width, self.height = width, height

    def generate_density_grid(self, n_iterations: int = 16, decay: float = 0.95) -> float:
        """nrf_generate_density_grid; returns the new mean_density."""
        m = C.c_float()
        _check(self.lib.nrf_generate_density_grid(self.h, int(n_iterations), C.c_float(decay), C.byref(m)))
        return float(m.value)

    def read_density_grid(self, n_cells: int):
        grid = np.empty(n_cells, np.float32)
        m = C.c_float()
        _check(self.lib.nrf_read_density_grid(self.h, grid.ctypes.data, n_cells, C.byref(m)))
        return grid, float(m.value)

    def set_options(self, opts: Options):
        _check(self.lib.nrf_set_options(self.h, C.byref(opts)))

    def render(self, cam, pose, stream=None) -> Frame:
        cam = np.ascontiguousarray(cam, dtype=np.float32).reshape(4)
        pose = np.ascontiguousarray(pose, dtype=np.float32).reshape(16)
        f = Frame()
        _check(self.lib.nrf_render(self.h, _fptr(cam), _fptr(pose), C.c_void_p(stream or 0), C.byref(f)))
        return f

    def set_max_views(self, n: int):
        _check(self.lib.nrf_set_max_views(self.h, int(n)))

    def render_views(self, cams, poses, stream=None) -> Frame:
        """nrf_render_views: cams [n][4], poses [n][4][4]; one launch per NRF_MAX_VIEWS views."""
        cams = np.ascontiguousarray(cams, dtype=np.float32).reshape(-1, 4)
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
        if len(cams) != len(poses):
            raise ValueError("cams and poses must have the same length")
        f = Frame()
        _check(self.lib.nrf_render_views(self.h, len(cams), _fptr(cams), _fptr(poses), C.c_void_p(stream or 0), C.byref(f)))
        return f

    def render_rays(self, rays_o_ptr, rays_d_ptr, rays_per_view: int, n_views: int = 1, stream=None) -> Frame:
        """nrf_render_rays: frames from caller-supplied rays -- device fp32 [n_views][rays_per_view][3] origins and directions
        (ngp units, row-major pixels, as generate_rays writes them); pixels beyond rays_per_view and guarded rays are background."""
        f = Frame()
        _check(self.lib.nrf_render_rays(self.h, int(n_views), C.c_void_p(rays_o_ptr or 0), C.c_void_p(rays_d_ptr or 0),
                                        int(rays_per_view), C.c_void_p(stream or 0), C.byref(f)))
        return f

    def render_rays_clipped(self, rays_o_ptr, rays_d_ptr, rays_per_view: int, t_min_ptr=0, t_max_ptr=0, background_ptr=0,
                            flags: int = 0, n_views: int = 1, stream=None) -> Frame:
        """nrf_render_rays_clipped: render_rays between per-ray limits of t -- device fp32 [n_views][rays_per_view] each, in units
        of t along the (not normalised) direction; a NaN entry, or a null pointer (0) for the whole array: no limit (an ENTRY of 0 is a
        limit like any other: t_max = 0 empties the ray) -- over a per-ray background, device fp32
        [n_views][rays_per_view][3] (0: the scalar bg_color).  flags: NRF_RAYS_DEPTH_T = the depth plane is the composited sum of
        w * t (divide by alpha for the expected hit distance) instead of the normalised depth; NRF_RAYS_DENSITY_ONLY (may be combined
        with it; float outputs only) = shadow / occlusion rays: the density network alone is evaluated, alpha and depth are those of
        the call without the flag bit for bit, and rgb = (1 - alpha) * background (the ray's entry, or bg_color) -- pass the light's
        unshadowed radiance as background and its distance over |d| as t_max."""
        r = Rays(rays_o_ptr or None, rays_d_ptr or None, int(rays_per_view), t_min_ptr or None, t_max_ptr or None,
                 background_ptr or None, int(flags), 0)
        f = Frame()
        _check(self.lib.nrf_render_rays_clipped(self.h, int(n_views), C.byref(r), C.c_void_p(stream or 0), C.byref(f)))
        return f

    def ray_hits(self, rays_o_ptr, rays_d_ptr, rays_per_view: int, opacity: float, t_min_ptr=0, t_max_ptr=0, n_views: int = 1,
                 stream=None) -> Frame:
        """nrf_ray_hits: where each ray's weight sum first reaches `opacity` (0 < opacity <= 1) -- the rays, t_min and t_max as in
        render_rays_clipped, processed as its NRF_RAYS_DENSITY_ONLY mode processes them, and stopped at the first sample whose updated
        weight sum is >= opacity.  rgba of a hit: (t of that sample as composited, its dt, the weight sum before it, the weight sum
        after it); of a miss: (0, 0, 0, the final weight sum < opacity); without a ray: zeros.  depth: the sum of w * t as composited
        (NRF_RAYS_DEPTH_T semantics).  Float outputs only; no background takes part."""
        r = Rays(rays_o_ptr or None, rays_d_ptr or None, int(rays_per_view), t_min_ptr or None, t_max_ptr or None, None, 0, 0)
        f = Frame()
        _check(self.lib.nrf_ray_hits(self.h, int(n_views), C.byref(r), C.c_float(opacity), C.c_void_p(stream or 0), C.byref(f)))
        return f

    def read_view_f32(self, view: int):
        rgba = np.empty((self.height, self.width, 4), np.float32)
        depth = np.empty((self.height, self.width), np.float32)
        _check(self.lib.nrf_read_view_f32(self.h, int(view), rgba.ctypes.data, depth.ctypes.data))
        return rgba, depth

    def read_view_u8(self, view: int):
        rgb = np.empty((self.height, self.width, 3), np.uint8)
        depth = np.empty((self.height, self.width), np.uint8)
        _check(self.lib.nrf_read_view_u8(self.h, int(view), rgb.ctypes.data, depth.ctypes.data))
        return rgb, depth

    def bind_output(self, rgba_ptr, depth_ptr):
        _check(self.lib.nrf_bind_output(self.h, C.c_void_p(rgba_ptr or 0), C.c_void_p(depth_ptr or 0)))

    def bind_output_rgbd8(self, rgbd8_ptr):
        """Packed 8-bit target (r | g << 8 | b << 16 | depth << 24 per pixel) of subsequent renders; 0: back to the float planes."""
        _check(self.lib.nrf_bind_output_rgbd8(self.h, C.c_void_p(rgbd8_ptr or 0)))

    def bind_output_u8(self, rgb8_ptr, depth8_ptr):
        """8-bit planar targets (the reference's Image layout) of subsequent renders; 0, 0: back to the float planes."""
        _check(self.lib.nrf_bind_output_u8(self.h, C.c_void_p(rgb8_ptr or 0), C.c_void_p(depth8_ptr or 0)))

    # ---- host frames: render_frame's result in (pinned) host memory
    def submit_host_u8(self, cams, poses, flags: int = 0) -> int:
        cams, poses = _views(cams, poses)
        t = C.c_int(-1)
        _check(self.lib.nrf_submit_host_u8(self.h, len(cams), _fptr(cams), _fptr(poses), int(flags), C.byref(t)))
        return int(t.value)

    def wait_host_u8(self, ticket: int, copy: bool = True):
        """(rgb u8 [n][H][W][3], depth u8 [n][H][W] or None); copy=False: views of the context's pinned memory, valid
        until the second next submit."""
        f = HostFrame()
        _check(self.lib.nrf_wait_host_u8(self.h, int(ticket), C.byref(f)))
        return _host_frame_arrays(f, copy)

    def render_host_u8(self, cams, poses, flags: int = 0, copy: bool = True):
        cams, poses = _views(cams, poses)
        f = HostFrame()
        _check(self.lib.nrf_render_host_u8(self.h, len(cams), _fptr(cams), _fptr(poses), int(flags), C.byref(f)))
        return _host_frame_arrays(f, copy)

    def render_host_u8_raw(self, cams, poses, flags: int = 0) -> HostFrame:
        """nrf_render_host_u8 with prepared float32 arrays (cams [n][4], poses [n][16]); returns the HostFrame itself
        (pointers into the context's pinned memory, render_ms, copied_bytes): the timing form bench.py uses."""
        f = HostFrame()
        _check(self.lib.nrf_render_host_u8(self.h, len(cams), _fptr(cams), _fptr(poses), int(flags), C.byref(f)))
        return f

    def read_f32(self):
        rgba = np.empty((self.height, self.width, 4), np.float32)
        depth = np.empty((self.height, self.width), np.float32)
        _check(self.lib.nrf_read_f32(self.h, rgba.ctypes.data, depth.ctypes.data))
        return rgba, depth

    def read_u8(self):
        rgb = np.empty((self.height, self.width, 3), np.uint8)
        depth = np.empty((self.height, self.width), np.uint8)
        _check(self.lib.nrf_read_u8(self.h, rgb.ctypes.data, depth.ctypes.data))
        return rgb, depth

    def stats(self) -> Stats:
        s = Stats()
        _check(self.lib.nrf_get_stats(self.h, C.byref(s)))
        return s

    def untile(self, gathered_ptr, shard_count, tiles, channels, out_ptr, stream=None):
        _check(self.lib.nrf_untile(self.h, C.c_void_p(gathered_ptr), shard_count, tiles, channels,
                                   C.c_void_p(out_ptr), C.c_void_p(stream or 0)))

    def quantize_rgbd8(self, rgba_ptr, depth_ptr, n_px, out_ptr, stream=None):
        _check(self.lib.nrf_quantize_rgbd8(self.h, C.c_void_p(rgba_ptr), C.c_void_p(depth_ptr), int(n_px), C.c_void_p(out_ptr),
                                           C.c_void_p(stream or 0)))

    def quantize_u8(self, rgba_ptr, depth_ptr, n_px, rgb8_ptr, depth8_ptr, stream=None):
        _check(self.lib.nrf_quantize_u8(self.h, C.c_void_p(rgba_ptr), C.c_void_p(depth_ptr), int(n_px), C.c_void_p(rgb8_ptr),
                                        C.c_void_p(depth8_ptr), C.c_void_p(stream or 0)))

    def untile_views_u8(self, gathered_ptr, shard_count, tiles, n_views, rgb8_ptr, depth8_ptr, stream=None):
        _check(self.lib.nrf_untile_views_u8(self.h, C.c_void_p(gathered_ptr), shard_count, tiles, n_views, C.c_void_p(rgb8_ptr),
                                            C.c_void_p(depth8_ptr), C.c_void_p(stream or 0)))

    def untile_views(self, gathered_ptr, shard_count, tiles, channels, n_views, out_ptr, stream=None):
        _check(self.lib.nrf_untile_views(self.h, C.c_void_p(gathered_ptr), shard_count, tiles, channels, n_views,
                                         C.c_void_p(out_ptr), C.c_void_p(stream or 0)))

    # ---- stage entry points; arguments are device pointers (ints) ----
    def encode_grid(self, pos01, n, out, stream=None):
        _check(self.lib.nrf_encode_grid(self.h, C.c_void_p(pos01), n, C.c_void_p(out), C.c_void_p(stream or 0)))

    def encode_dir(self, dir01, n, out, stream=None):
        _check(self.lib.nrf_encode_dir(self.h, C.c_void_p(dir01), n, C.c_void_p(out), C.c_void_p(stream or 0)))

    def mlp_forward(self, feat, dirfeat, n, out, stream=None):
        _check(self.lib.nrf_mlp_forward(self.h, C.c_void_p(feat), C.c_void_p(dirfeat), n, C.c_void_p(out),
                                        C.c_void_p(stream or 0)))

    def mlp_forward_repeat(self, feat, dirfeat, n, out, repeat, stream=None):
        _check(self.lib.nrf_mlp_forward_repeat(self.h, C.c_void_p(feat), C.c_void_p(dirfeat), n, C.c_void_p(out), int(repeat),
                                               C.c_void_p(stream or 0)))

    def network(self, xyz, dirs, n, sigma, rgb, stream=None):
        _check(self.lib.nrf_network(self.h, C.c_void_p(xyz), C.c_void_p(dirs), n, C.c_void_p(sigma), C.c_void_p(rgb),
                                    C.c_void_p(stream or 0)))

    def density(self, xyz, n, sigma, stream=None):
        """nrf_density: sigma of the density network alone at n points (device fp32 [n][3] -> [n]) -- nrf_network's sigma bit for
        bit; a point with a coordinate that is not finite or outside [-bound, bound] yields 0."""
        _check(self.lib.nrf_density(self.h, C.c_void_p(xyz), int(n), C.c_void_p(sigma), C.c_void_p(stream or 0)))

    def density_gradient(self, xyz, n, h, out, stream=None):
        """nrf_density_gradient: out (device float4 [n]) = (g_x, g_y, g_z, sigma), g_k = (sigma(x + h e_k) - sigma(x - h e_k)) *
        fp32(1 / (h + h)); a point with any tap coordinate not finite or outside [-bound, bound] yields zeros.  The surface normal
        is normals_from_gradients(out)."""
        _check(self.lib.nrf_density_gradient(self.h, C.c_void_p(xyz), int(n), C.c_float(h), C.c_void_p(out), C.c_void_p(stream or 0)))

    def hit_gradients(self, hits: Frame, rays_o_ptr, rays_d_ptr, rays_per_view: int, opacity: float, frac: float, h: float, pos, out,
                      stream=None):
        """nrf_hit_gradients: the gradient records at the hits of the nrf_ray_hits frame `hits` (row-major), for the rays it was
        made from.  pos, out: device float4 [hits.n_views * hits.view_stride_px]; a hit pixel gets pos = (x, y, z, tq) with
        tq = t - frac * dt, x = o + tq d, and out = the record of density_gradient at x; every other pixel zeros."""
        r = Rays(rays_o_ptr or None, rays_d_ptr or None, int(rays_per_view), None, None, None, 0, 0)
        _check(self.lib.nrf_hit_gradients(self.h, C.byref(hits), C.byref(r), C.c_float(opacity), C.c_float(frac), C.c_float(h),
                                          C.c_void_p(pos), C.c_void_p(out), C.c_void_p(stream or 0)))

    def density_lattice(self, lattice: Lattice, sigma, stream=None):
        """nrf_density_lattice: sigma (device fp32 [nx][ny][nz]) at every point of the lattice, bit-identical to density() on the
        positions origin + (float)index * cell; 0 where a coordinate is outside [-bound, bound].  No positions are uploaded."""
        _check(self.lib.nrf_density_lattice(self.h, C.byref(lattice), C.c_void_p(sigma), C.c_void_p(stream or 0)))

    def extract_mesh(self, lattice: Lattice, iso: float, sigma=None, stream=None) -> Mesh:
        """nrf_extract_mesh: the iso-surface sigma == iso of the lattice by marching tetrahedra, on the device.  sigma None: the
        model is evaluated on the lattice; otherwise the caller's device array [nx][ny][nz] is polygonised (no model needed).
        Returns after completion.  mesh.vertices is [n][3]: density_gradient(mesh.vertices, mesh.n_vertices, h, out) takes it as it
        is, and normals_from_gradients(out) are the vertex normals."""
        out = Mesh()
        _check(self.lib.nrf_extract_mesh(self.h, C.byref(lattice), C.c_float(iso), C.c_void_p(sigma or 0), C.c_void_p(stream or 0),
                                         C.byref(out)))
        self._mesh_counts = (int(out.n_vertices), int(out.n_triangles))
        return out

    def read_mesh(self):
        """nrf_read_mesh: (vertices float32 [n_vertices][3], triangles uint32 [n_triangles][3]) of the last extract_mesh"""
        nv, nt = getattr(self, "_mesh_counts", (0, 0))
        v, t = np.empty((nv, 3), np.float32), np.empty((nt, 3), np.uint32)
        _check(self.lib.nrf_read_mesh(self.h, v.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_uint32))))
        return v, t

    def point_attributes(self, xyz_ptr, n, h, normal_ptr, color_ptr, dir_ptr=0, stream=None):
        """nrf_point_attributes: normal (device float4 [n]) = (n_x, n_y, n_z, sigma), color (device float4 [n]) = (r, g, b, |g|) at n
        points (device fp32 [n][3]): n = -g / |g| of density_gradient's record, sigma and rgb those of network() at the point, looked
        at along dir (device fp32 [n][3]) or, dir_ptr 0, along -n.  A point the guard of density_gradient refuses yields zeros."""
        _check(self.lib.nrf_point_attributes(self.h, C.c_void_p(xyz_ptr), C.c_void_p(dir_ptr or 0), int(n), C.c_float(h),
                                             C.c_void_p(normal_ptr), C.c_void_p(color_ptr), C.c_void_p(stream or 0)))

    def mesh_attributes(self, h: float, stream=None) -> MeshAttr:
        """nrf_mesh_attributes: point_attributes at the vertices of the last extract_mesh, into buffers of the context.  Returns
        after completion."""
        out = MeshAttr()
        _check(self.lib.nrf_mesh_attributes(self.h, C.c_float(h), C.c_void_p(stream or 0), C.byref(out)))
        self._mesh_attr_count = int(out.n_vertices)
        return out

    def read_mesh_attributes(self):
        """nrf_read_mesh_attributes: (normals float32 [n_vertices][4], colors float32 [n_vertices][4]) of the last mesh_attributes"""
        nv = getattr(self, "_mesh_attr_count", 0)
        nrm, col = np.empty((nv, 4), np.float32), np.empty((nv, 4), np.float32)
        _check(self.lib.nrf_read_mesh_attributes(self.h, nrm.ctypes.data_as(C.POINTER(C.c_float)), col.ctypes.data_as(C.POINTER(C.c_float))))
        return nrm, col

    def mesh_components(self, stream=None) -> MeshParts:
        """nrf_mesh_components: the connected components of the current mesh, labelled on the device: parts.labels (uint32
        [n_vertices], the smallest vertex id of each vertex's component) and parts.components (uint32 [n_components][3] = (label,
        n_vertices, n_triangles), ascending label), in buffers of the context.  Returns after completion."""
        out = MeshParts()
        _check(self.lib.nrf_mesh_components(self.h, C.c_void_p(stream or 0), C.byref(out)))
        self._mesh_parts_counts = (getattr(self, "_mesh_counts", (0, 0))[0], int(out.n_components))
        return out

    def read_mesh_components(self):
        """nrf_read_mesh_components: (labels uint32 [n_vertices], components uint32 [n_components][3]) of the last mesh_components"""
        nv, nc = getattr(self, "_mesh_parts_counts", (0, 0))
        labels, table = np.empty(nv, np.uint32), np.empty((nc, 3), np.uint32)
        _check(self.lib.nrf_read_mesh_components(self.h, labels.ctypes.data_as(C.POINTER(C.c_uint32)), table.ctypes.data_as(C.POINTER(C.c_uint32))))
        return labels, table

    def filter_mesh(self, min_triangles: int = 0, keep_largest: bool = False, stream=None) -> Mesh:
        """nrf_filter_mesh: keeps the components of the current mesh with at least min_triangles triangles -- with keep_largest only
        the one with the most triangles, a tie going to the smaller label -- and makes the result the context's mesh: read_mesh and
        mesh_attributes see it.  The labelling and the attributes of the mesh it replaced are invalid afterwards."""
        out = Mesh()
        _check(self.lib.nrf_filter_mesh(self.h, C.c_uint64(int(min_triangles)), C.c_uint32(NRF_MESH_KEEP_LARGEST if keep_largest else 0),
                                        C.c_void_p(stream or 0), C.byref(out)))
        self._mesh_counts = (int(out.n_vertices), int(out.n_triangles))
        self._mesh_parts_counts = (0, 0)
        return out

    def refine_mesh(self, n_steps: int, stream=None) -> MeshRefine:
        """nrf_refine_mesh: moves every vertex of the current mesh along its lattice edge onto the iso value of the density network --
        n_steps (0 .. 16) bisections and one secant step, in one launch -- and rewrites the vertices in place.  Triangles and a current
        labelling stay valid; the attributes are invalid afterwards.  Returns after completion; out.n_unbracketed counts the vertices
        whose edge does not bracket iso (a caller's lattice that disagrees with the network): they keep their bits."""
        out = MeshRefine()
        _check(self.lib.nrf_refine_mesh(self.h, C.c_uint32(int(n_steps)), C.c_void_p(stream or 0), C.byref(out)))
        return out

    def read_mesh_refinement(self, brackets: bool = True):
        """nrf_read_mesh_refinement: (edges uint32 [n_vertices] = (p << 3) | m, brackets float32 [n_vertices][4] = (lo, hi, s_lo, s_hi))
        of the current mesh.  The edge words exist after any extract_mesh or filter_mesh; the brackets only after a refine_mesh of the
        current mesh -- brackets=False reads the edge words alone and returns (edges, None)."""
        nv = getattr(self, "_mesh_counts", (0, 0))[0]
        e = np.empty(nv, np.uint32)
        b = np.empty((nv, 4), np.float32) if brackets else None
        _check(self.lib.nrf_read_mesh_refinement(self.h, e.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 b.ctypes.data_as(C.POINTER(C.c_float)) if brackets else None))
        return e, b

    def simplify_mesh(self, factor: int, stream=None) -> MeshSimplify:
        """nrf_simplify_mesh: merges the vertices of the current mesh whose lattice points share a block of factor^3 points (factor
        1 .. 256) into the one nearest the block's centre, drops the triangles that collapse and the vertices nothing names any more,
        and makes the result the context's mesh: read_mesh, filter_mesh, refine_mesh and mesh_attributes see it.  Every vertex of the
        result is an old vertex, bit for bit, with its edge word.  The labelling, the attributes and the brackets of the mesh it
        replaced are invalid afterwards.  Returns after completion."""
        out = MeshSimplify()
        _check(self.lib.nrf_simplify_mesh(self.h, C.c_uint32(int(factor)), C.c_void_p(stream or 0), C.byref(out)))
        self._mesh_counts = (int(out.n_vertices), int(out.n_triangles))
        self._mesh_parts_counts = (0, 0)
        self._mesh_simplify_counts = (int(out.n_vertices), int(out.n_vertices_before))
        return out

    def read_mesh_simplification(self):
        """nrf_read_mesh_simplification: (sources uint32 [n_vertices] = the old id of every vertex of the simplified mesh, ascending,
        vertex_map uint32 [n_vertices_before] = the new id of every old vertex's representative, or 0xffffffff) of the last
        simplify_mesh of the current mesh"""
        nv, before = getattr(self, "_mesh_simplify_counts", (0, 0))
        src, vmap = np.empty(nv, np.uint32), np.empty(before, np.uint32)
        _check(self.lib.nrf_read_mesh_simplification(self.h, src.ctypes.data_as(C.POINTER(C.c_uint32)), vmap.ctypes.data_as(C.POINTER(C.c_uint32))))
        return src, vmap

    def bake_mesh_texture(self, res: int, width: int, stream=None) -> MeshTexture:
        """nrf_bake_mesh_texture: the colours of the full network on a per-triangle texture atlas of the current mesh -- res texels
        along a triangle's legs (2 .. 256), two triangles per cell of (res + 2) x (res + 1) texels, width / (res + 2) cells per atlas
        row -- into buffers of the context: texels float4 [height][width] = (r, g, b, sigma), rgba8 uint32 [height][width] (alpha 255
        where a triangle's texel was evaluated, 0 elsewhere) and uvs float [n_triangles][3][2].  The mesh is only read.  Returns after
        completion; out.n_refused counts the texels of existing triangles that the guard zeroed."""
        out = MeshTexture()
        _check(self.lib.nrf_bake_mesh_texture(self.h, C.c_uint32(int(res)), C.c_uint32(int(width)), C.c_void_p(stream or 0), C.byref(out)))
        self._mesh_texture_shape = (int(out.height), int(out.width), int(out.n_triangles))
        return out

    def read_mesh_texture(self):
        """nrf_read_mesh_texture: (texels float32 [H][W][4], rgba8 uint32 [H][W], uvs float32 [T][3][2]) of the last bake_mesh_texture
        of the current mesh"""
        h, w, nt = getattr(self, "_mesh_texture_shape", (0, 0, 0))
        tex, rgba, uvs = np.empty((h, w, 4), np.float32), np.empty((h, w), np.uint32), np.empty((nt, 3, 2), np.float32)
        _check(self.lib.nrf_read_mesh_texture(self.h, tex.ctypes.data_as(C.POINTER(C.c_float)), rgba.ctypes.data_as(C.POINTER(C.c_uint32)),
                                              uvs.ctypes.data_as(C.POINTER(C.c_float))))
        return tex, rgba, uvs

    def generate_rays(self, cam, pose, rays_o, rays_d, nears, fars, stream=None):
        cam = np.ascontiguousarray(cam, dtype=np.float32).reshape(4)
        pose = np.ascontiguousarray(pose, dtype=np.float32).reshape(16)
        _check(self.lib.nrf_generate_rays(self.h, _fptr(cam), _fptr(pose), C.c_void_p(rays_o), C.c_void_p(rays_d),
                                          C.c_void_p(nears), C.c_void_p(fars), C.c_void_p(stream or 0)))

    def motion_vectors(self, rays_o, rays_d, rgba, depth_t, width, height, out_width, out_height, cam, pose, prev_cam, prev_pose, out,
                       min_alpha=0.5, stream=None, reserved=0):
        """the motion vectors of a static scene (nrf_motion_vectors): device planes of a NRF_RAYS_DEPTH_T ray frame and its rays ->
        device float2 [height][width] in output pixels, what RenderBuffer.upscale_temporal takes as `motion`."""
        m = Motion()
        m.rays_o, m.rays_d, m.rgba, m.depth_t = rays_o, rays_d, rgba, depth_t
        m.width, m.height, m.out_width, m.out_height = width, height, out_width, out_height
        m.min_alpha, m.reserved = min_alpha, reserved
        m.cam[:] = [float(v) for v in np.asarray(cam, np.float32).reshape(4)]
        m.pose[:] = [float(v) for v in np.asarray(pose, np.float32).reshape(16)]
        m.prev_cam[:] = [float(v) for v in np.asarray(prev_cam, np.float32).reshape(4)]
        m.prev_pose[:] = [float(v) for v in np.asarray(prev_pose, np.float32).reshape(16)]
        _check(self.lib.nrf_motion_vectors(self.h, C.byref(m), C.c_void_p(out or 0), C.c_void_p(stream or 0)))

    def march(self, rays_o, rays_d, rays_t, fars, n, n_step, xyzs, dirs, deltas, stream=None):
        _check(self.lib.nrf_march(self.h, C.c_void_p(rays_o), C.c_void_p(rays_d), C.c_void_p(rays_t), C.c_void_p(fars),
                                  n, n_step, C.c_void_p(xyzs), C.c_void_p(dirs), C.c_void_p(deltas),
                                  C.c_void_p(stream or 0)))

    def composite(self, sigmas, rgbs, deltas, n, n_step, rays_t, state, stream=None):
        _check(self.lib.nrf_composite(self.h, C.c_void_p(sigmas), C.c_void_p(rgbs), C.c_void_p(deltas), n, n_step,
                                      C.c_void_p(rays_t), C.c_void_p(state), C.c_void_p(stream or 0)))


def normals_from_gradients(out):
    """Surface normals of gradient records (nrf_density_gradient / nrf_hit_gradients: [..., 4] = g_x, g_y, g_z, sigma): -g / |g|,
    and zero where |g| == 0 (a refused point, a miss, a flat spot)."""
    g = np.asarray(out, np.float32)[..., :3]
    norm = np.sqrt(np.sum(g.astype(np.float64) ** 2, axis=-1, keepdims=True))
    return np.where(norm > 0, -g / np.where(norm > 0, norm, 1.0), 0.0).astype(np.float32)


CS_LINEAR, CS_SRGB, CS_VISPOSNEG = 0, 1, 2
TM_IDENTITY, TM_ACES, TM_HABLE, TM_REINHARD = 0, 1, 2, 3
IMG_BYTE, IMG_HALF, IMG_FLOAT = 1, 2, 3  # EImageDataType: uint32 sRGB texels with straight alpha, four fp16, four fp32


class NerfGroup:
    """nrf_group: several devices driven by this process (the reference's NGPU, common.h:91)."""

    def __init__(self, devices):
        self.lib = load_library()
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        _check(self.lib.nrf_group_create(len(devices), devs, C.byref(h)))
        self.h = h
        self.width = self.height = 0

    def close(self):
        if self.h:
            self.lib.nrf_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def load_model(self, desc):
        _check(self.lib.nrf_group_load_model(self.h, C.byref(desc)))

    def set_gather(self, mode: int):
        """The transport of the exchange step: GATHER_PEER_COPY (hipMemcpyPeerAsync) or GATHER_RCCL (ncclSend / ncclRecv to
        devices[0]; a one-member group then runs the whole exchange too)."""
        _check(self.lib.nrf_group_set_gather(self.h, int(mode)))

    def gather(self):
        """(mode, RCCL version code or 0)"""
        m, v = C.c_int(), C.c_int()
        _check(self.lib.nrf_group_get_gather(self.h, C.byref(m), C.byref(v)))
        return int(m.value), int(v.value)

    def set_options(self, opts):
        _check(self.lib.nrf_group_set_options(self.h, C.byref(opts)))

    def generate_density_grid(self, n_iterations: int = 16, decay: float = 0.95) -> float:
        """Every member evaluates the density grid from its replica of the network (nrf_generate_density_grid)."""
        m = C.c_float()
        for i in range(self.lib.nrf_group_size(self.h)):
            ctx = C.c_void_p(self.lib.nrf_group_member(self.h, i))
            _check(self.lib.nrf_generate_density_grid(ctx, int(n_iterations), C.c_float(decay), C.byref(m)))
        return float(m.value)

    def set_resolution(self, width, height):
        _check(self.lib.nrf_group_set_resolution(self.h, width, height))
        self.width, self.height = width, height

    def render_views(self, cams, poses) -> Frame:
        cams = np.ascontiguousarray(cams, dtype=np.float32).reshape(-1, 4)
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
        f = Frame()
        _check(self.lib.nrf_group_render_views(self.h, len(cams), _fptr(cams), _fptr(poses), C.byref(f)))
        return f

    def read_view_f32(self, view):
        rgba = np.empty((self.height, self.width, 4), np.float32)
        depth = np.empty((self.height, self.width), np.float32)
        _check(self.lib.nrf_group_read_view_f32(self.h, int(view), rgba.ctypes.data, depth.ctypes.data))
        return rgba, depth

    def read_view_u8(self, view):
        rgb = np.empty((self.height, self.width, 3), np.uint8)
        depth = np.empty((self.height, self.width), np.uint8)
        _check(self.lib.nrf_group_read_view_u8(self.h, int(view), rgb.ctypes.data, depth.ctypes.data))
        return rgb, depth

    def submit_host_u8(self, cams, poses, flags: int = 0) -> int:
        cams, poses = _views(cams, poses)
        t = C.c_int(-1)
        _check(self.lib.nrf_group_submit_host_u8(self.h, len(cams), _fptr(cams), _fptr(poses), int(flags), C.byref(t)))
        return int(t.value)

    def wait_host_u8(self, ticket: int, copy: bool = True):
        f = HostFrame()
        _check(self.lib.nrf_group_wait_host_u8(self.h, int(ticket), C.byref(f)))
        return _host_frame_arrays(f, copy)

    def render_host_u8(self, cams, poses, flags: int = 0, copy: bool = True):
        cams, poses = _views(cams, poses)
        f = HostFrame()
        _check(self.lib.nrf_group_render_host_u8(self.h, len(cams), _fptr(cams), _fptr(poses), int(flags), C.byref(f)))
        return _host_frame_arrays(f, copy)

    def stats(self) -> Stats:
        s = Stats()
        _check(self.lib.nrf_group_get_stats(self.h, C.byref(s)))
        return s


class NerfRender:
    """Python mirror of ngp::NerfRender (reference include/nerf-cuda/nerf_render.h:29-50): the same method names
    and call order as the reference's testbed (src/main.cu:140-170), on an nrf_group of `n_gpus` devices.

        render = NerfRender()
        render.reload_network_from_file("snapshot.msgpack")
        render.set_resolution((1920, 1080))
        rgb, depth = render.render_frame(cam, pose)          # u8 [H][W][3], u8 [H][W]  (ngp::Image)
    """

    def __init__(self, n_gpus: int = 1, devices=None):
        self.group = NerfGroup(list(devices) if devices is not None else list(range(n_gpus)))
        self.network_config = None
        self.desc = None
        self._keep = None
        self.resolution = None

    def load_network_config(self, path):  # nerf_render.cu:66-91: .json or .msgpack
        path = str(path)
        if not os.path.exists(path):
            raise RuntimeError(f"Network config path {path} does not exist.")
        if path.lower().endswith(".json"):
            import json

            with open(path) as f:
                return json.load(f)
        import msgpack

        with open(path, "rb") as f:
            return msgpack.unpackb(f.read(), raw=False)

    def load_snapshot(self, path):  # nerf_render.cu:431-473
        config = self.load_network_config(path)
        if "snapshot" not in config:
            raise RuntimeError(f"File {path} does not contain a snapshot.")
        self.network_config = config

    def reset_network(self):  # nerf_render.cu:111-184
        self.desc, self._keep = desc_from_config(self.network_config)
        self.desc.gather_copy_budget_mb = int(getattr(self, "gather_copy_budget_mb", 0))  # 0: the library's default; 1: no gather copies

    def reload_network_from_file(self, path):  # nerf_render.cu:93-109
        self.load_snapshot(path)
        self.reset_network()
        self.group.load_model(self.desc)
        if self.desc.n_density_grid == 0:  # the snapshot carries no density grid
            self.generate_density_grid()

    def generate_density_grid(self):  # nerf_render.cu:388-429 (dead in the reference; see nrf_generate_density_grid)
        if self.desc is None:
            raise RuntimeError("generate_density_grid: no network loaded")
        self.desc.mean_density = self.group.generate_density_grid(16, 0.95)

    def set_resolution(self, resolution):  # nerf_render.cu:186-236
        self.resolution = (int(resolution[0]), int(resolution[1]))
        self.group.set_resolution(*self.resolution)

    def render_frame(self, cam, pos):  # nerf_render.cu:238-367
        return self.render_frames([cam], [pos])[0]

    def render_frames(self, cams, poses):
        """Batched form: one launch per NRF_MAX_VIEWS cameras and device; [(rgb u8, depth u8), ...]."""
        if self.desc is None or self.resolution is None:
            raise RuntimeError("reload_network_from_file and set_resolution must be called first")
        # the kernel writes the Image's bytes itself; they arrive in pinned host memory by one asynchronous copy
        rgb, depth = self.group.render_host_u8(cams, poses)
        return [(rgb[v], depth[v]) for v in range(len(rgb))]

    def close(self):
        self.group.close()


class RenderBuffer:
    """nrf_render_buffer: the presentation chain of the reference's CudaRenderBuffer (same method names)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        _check(self.lib.nrf_rb_create(device, C.byref(h)))
        self.h = h
        self.width = self.height = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.nrf_rb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def resize(self, width, height):
        _check(self.lib.nrf_rb_resize(self.h, width, height))
        self.width, self.height = width, height

    def reset_accumulation(self):
        _check(self.lib.nrf_rb_reset_accumulation(self.h))

    def spp(self):
        v = C.c_uint32()
        _check(self.lib.nrf_rb_spp(self.h, C.byref(v)))
        return int(v.value)

    def set_color_space(self, cs):
        _check(self.lib.nrf_rb_set_color_space(self.h, cs))

    def set_tonemap_curve(self, curve):
        _check(self.lib.nrf_rb_set_tonemap_curve(self.h, curve))

    def buffers(self):
        f, d, a, s = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self.lib.nrf_rb_buffers(self.h, C.byref(f), C.byref(d), C.byref(a), C.byref(s)))
        return f.value, d.value, a.value, s.value

    def clear_frame(self, stream=None):
        _check(self.lib.nrf_rb_clear_frame(self.h, C.c_void_p(stream or 0)))

    def accumulate(self, exposure=0.0, stream=None):
        _check(self.lib.nrf_rb_accumulate(self.h, C.c_float(exposure), C.c_void_p(stream or 0)))

    def tonemap(self, exposure, background_color, output_color_space, stream=None):
        bg = np.ascontiguousarray(background_color, np.float32).reshape(4)
        _check(self.lib.nrf_rb_tonemap(self.h, C.c_float(exposure), _fptr(bg), output_color_space, C.c_void_p(stream or 0)))

    def present(self, exposure, background_color, output_color_space, rgba8_ptr=None, stream=None):
        """accumulate() + tonemap() in one pass over the planes (nrf_rb_present); rgba8_ptr: optional device uint32 [h][w]."""
        bg = np.ascontiguousarray(background_color, np.float32).reshape(4)
        _check(self.lib.nrf_rb_present(self.h, C.c_float(exposure), _fptr(bg), output_color_space, C.c_void_p(rgba8_ptr or 0),
                                       C.c_void_p(stream or 0)))

    def overlay_depth(self, alpha, depth_ptr, depth_scale, image_width, image_height, fov_axis=0, zoom=1.0,
                      screen_center=(0.5, 0.5), stream=None):
        ctr = np.ascontiguousarray(screen_center, np.float32).reshape(2)
        _check(self.lib.nrf_rb_overlay_depth(self.h, C.c_float(alpha), C.c_void_p(depth_ptr), C.c_float(depth_scale), image_width,
                                             image_height, fov_axis, C.c_float(zoom), _fptr(ctr), C.c_void_p(stream or 0)))

    def overlay_image(self, alpha, exposure, background_color, output_color_space, image_ptr, image_data_type, image_width, image_height,
                      fov_axis=0, zoom=1.0, screen_center=(0.5, 0.5), stream=None):
        """a device image of IMG_BYTE / IMG_HALF / IMG_FLOAT texels over its background, developed and blended over the surface with
        weight alpha (nrf_rb_overlay_image); exposure: one value or one per channel"""
        e = np.ascontiguousarray(np.broadcast_to(np.asarray(exposure, np.float32), (3,)))
        bg = np.ascontiguousarray(background_color, np.float32).reshape(4)
        ctr = np.ascontiguousarray(screen_center, np.float32).reshape(2)
        _check(self.lib.nrf_rb_overlay_image(self.h, C.c_float(alpha), _fptr(e), _fptr(bg), output_color_space, C.c_void_p(image_ptr or 0),
                                             image_data_type, image_width, image_height, fov_axis, C.c_float(zoom), _fptr(ctr),
                                             C.c_void_p(stream or 0)))

    def overlay_false_color(self, training_width, training_height, fov_axis, error_map_ptr, map_width, map_height, average_ptr,
                            brightness=1.0, viridis=True, stream=None):
        """the surface's grey times the colour map of a device error map over its average (nrf_rb_overlay_false_color)"""
        _check(self.lib.nrf_rb_overlay_false_color(self.h, training_width, training_height, fov_axis, C.c_void_p(error_map_ptr or 0),
                                                   map_width, map_height, C.c_void_p(average_ptr or 0), C.c_float(brightness),
                                                   int(bool(viridis)), C.c_void_p(stream or 0)))

    def error_map(self, truth_ptr, map_width, map_height, error_map_ptr, average_ptr, stream=None):
        """the per-cell mean squared error of the surface against a device float4 truth plane, and the mean of the cells
        (nrf_rb_error_map); error_map_ptr: device float [map_height][map_width], average_ptr: one device float"""
        _check(self.lib.nrf_rb_error_map(self.h, C.c_void_p(truth_ptr or 0), map_width, map_height, C.c_void_p(error_map_ptr or 0),
                                         C.c_void_p(average_ptr or 0), C.c_void_p(stream or 0)))

    def host_to_accumulate_buffer(self, rgb_u8):
        rgb = np.ascontiguousarray(rgb_u8, np.uint8)
        _check(self.lib.nrf_rb_host_to_accumulate_buffer(self.h, rgb.ctypes.data, rgb.size // 3))

    def read(self):
        acc = np.empty((self.height, self.width, 4), np.float32)
        sur = np.empty((self.height, self.width, 4), np.float32)
        _check(self.lib.nrf_rb_read(self.h, acc.ctypes.data, sur.ctypes.data))
        return acc, sur

    # the upscaler: where the reference's render buffer has DLSS (enable_dlss, set_dlss_sharpening, in_/out_resolution); a spatial
    # bicubic reconstruction and a clamped unsharp mask in one launch, defined in include/nerfhip.h so that a host replays it
    def enable_upscale(self, out_width, out_height):
        _check(self.lib.nrf_rb_enable_upscale(self.h, out_width, out_height))

    def disable_upscale(self):
        _check(self.lib.nrf_rb_disable_upscale(self.h))

    def set_upscale_sharpening(self, amount):
        _check(self.lib.nrf_rb_set_upscale_sharpening(self.h, C.c_float(amount)))

    def resolutions(self):
        """((in_width, in_height), (out_width, out_height)); out == in while upscaling is disabled"""
        i, o = (C.c_int * 2)(), (C.c_int * 2)()
        _check(self.lib.nrf_rb_resolutions(self.h, i, o))
        return (int(i[0]), int(i[1])), (int(o[0]), int(o[1]))

    def upscale(self, rgba8_ptr=None, stream=None):
        """the surface as it is -> the upscaled plane (nrf_rb_upscale); rgba8_ptr: optional device uint32 [out_h][out_w]."""
        _check(self.lib.nrf_rb_upscale(self.h, C.c_void_p(rgba8_ptr or 0), C.c_void_p(stream or 0)))

    def upscaled_ptr(self):
        p = C.c_void_p()
        _check(self.lib.nrf_rb_upscaled(self.h, C.byref(p)))
        return p.value

    def read_upscaled(self):
        (_, _), (ow, oh) = self.resolutions()
        out = np.empty((oh, ow, 4), np.float32)
        _check(self.lib.nrf_rb_read_upscaled(self.h, out.ctypes.data))
        return out

    # the temporal upscaler: an accumulator at the output resolution over jittered frames (how the reference drives DLSS: jitter, a
    # reset flag, motion vectors), defined in include/nerfhip.h like the spatial one
    def set_upscale_history(self, max_history):
        _check(self.lib.nrf_rb_set_upscale_history(self.h, C.c_float(max_history)))

    def upscale_temporal(self, jitter, motion=None, reset=False, rectify=False, rgba8=None, stream=None, flags=0, reserved=0):
        """the surface as it is, sampled with `jitter`, into the history and the upscaled plane (nrf_rb_upscale_temporal); motion: optional
        device float2 [in_h][in_w] in output pixels; rgba8: optional device uint32 [out_h][out_w]."""
        t = UpscaleTemporal()
        t.motion = motion or None
        t.jitter[0], t.jitter[1] = float(jitter[0]), float(jitter[1])
        t.flags = flags | (NRF_UPSCALE_T_RESET if reset else 0) | (NRF_UPSCALE_T_RECTIFY if rectify else 0)
        t.reserved = reserved
        _check(self.lib.nrf_rb_upscale_temporal(self.h, C.byref(t), C.c_void_p(rgba8 or 0), C.c_void_p(stream or 0)))

    def upscale_history(self):
        """(history device pointer, weight device pointer, n_frames) as the last upscale_temporal left them"""
        h, w, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
        _check(self.lib.nrf_rb_upscale_history(self.h, C.byref(h), C.byref(w), C.byref(n)))
        return h.value, w.value, int(n.value)

    def read_upscale_history(self):
        """(H' float32 [out_h][out_w][4], Wt' float32 [out_h][out_w]) of the last upscale_temporal"""
        (_, _), (ow, oh) = self.resolutions()
        rgba, weight = np.empty((oh, ow, 4), np.float32), np.empty((oh, ow), np.float32)
        _check(self.lib.nrf_rb_read_upscale_history(self.h, rgba.ctypes.data, weight.ctypes.data))
        return rgba, weight


# --------------------------------------------------------------------------
# tile partition of one frame over ranks (host-side mirror of render_kernel's mapping and of
# untile_kernel): a strip = 4 horizontally adjacent 8x8 tiles; strip id = ty*strips_x + tx//4 belongs to
# rank strip % world as local strip strip // world; local tile = 4*local strip + tx % 4
# --------------------------------------------------------------------------
def shard_tile_ids(width: int, height: int, rank: int, world: int):
    """(tx, ty) of this rank's local tiles, in local order; padding tiles of a ragged strip included."""
    tiles_x, tiles_y = (width + 7) // 8, (height + 7) // 8
    strips_x = (tiles_x + 3) // 4
    out = []
    for strip in range(rank, strips_x * tiles_y, world):
        for j in range(4):
            out.append(((strip % strips_x) * 4 + j, strip // strips_x))
    return out


def untile_numpy(gathered: np.ndarray, width: int, height: int):
    """gathered [world][tiles_per_shard*64][C] (every rank's tile-major shard) -> [H][W][C]."""
    world = gathered.shape[0]
    strips_x = ((width + 7) // 8 + 3) // 4
    ys, xs = np.mgrid[0:height, 0:width]
    tx, ty = xs // 8, ys // 8
    strip = ty * strips_x + tx // 4
    lane = (ys % 8) * 8 + xs % 8
    return gathered[strip % world, ((strip // world) * 4 + tx % 4) * 64 + lane]
