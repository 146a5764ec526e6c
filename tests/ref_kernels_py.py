"""ctypes binding of oracle/_ref/libref_kernels.so and a Python restatement of render_frame's loop -- TEST INFRASTRUCTURE ONLY.

The library is the reference's own ray set-up, march, compaction and compositing kernels compiled for the CPU
(oracle/ref_kernels.cpp, `make -C oracle ref`).  It needs a reference tree at build time and is never committed, so:
  * where the tree exists and the library does not, `require()` FAILS (the build is broken);
  * where neither exists, `require()` skips (there is nothing to compare with: the committed golden vectors of
    tests/golden/reference_kernels.npz stand in, tests/test_reference_kernels_gpu.py).

Array layouts are the reference's (R/src/nerf_render.cu:193-230; R = the reference tree): rays_o / rays_d planar [3][N], rays_alive
/ rays_t [2][N], xyzs / dirs [cap][3] and deltas [cap][2] (column-major 3 x cap and 2 x cap), image [N][3].  The reference deals
the pixels of a frame to NGPU = 2 devices as pixel = NGPU * tid + gpuid (render_utils.h:37): `halves()` runs both."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "oracle" / "_ref" / "libref_kernels.so"
REFERENCE = Path(os.environ.get("REFERENCE", "/root/reference"))
THREADS = 128  # m_num_thread, nerf_render.h:77
FLT_MAX = np.float32(np.finfo(np.float32).max)
_lib = None


def reference_tree_exists() -> bool:
    return os.path.isfile(REFERENCE / "include" / "nerf-cuda" / "render_utils.h")  # False, not an error, where unreadable


def require():
    """The loaded library; a pytest failure where it should exist and does not, a skip where it cannot."""
    import pytest

    if not LIB.exists():
        if reference_tree_exists():
            pytest.fail(f"{LIB} is missing although the reference tree {REFERENCE} exists: run `make -C oracle ref` (build() does)")
        pytest.skip("no reference tree and no oracle/_ref/libref_kernels.so: nothing to hold the oracle to on this machine")
    return lib()


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = C.CDLL(str(LIB))
    vp, u32, i32, f32, f64 = C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_double
    sig = {
        "refk_ngpu": (i32, []),
        "refk_nerf_matrix_to_ngp": (None, [vp, f32, vp]),
        "refk_generate_rays": (None, [vp, vp, f32, i32, i32, i32, vp, vp]),
        "refk_near_far_from_aabb": (None, [vp, vp, vp, u32, f32, vp, vp]),
        "refk_init_step0": (None, [vp, vp, u32, i32, vp]),
        "refk_compact_rays": (i32, [i32, vp, vp, u32, i32, i32]),
        "refk_march_rays": (None, [u32, u32, vp, vp, u32, vp, vp, f32, f32, u32, u32, vp, f32, vp, vp, vp, vp, vp, u32, i32]),
        "refk_composite_rays": (None, [u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, i32]),
        "refk_get_image_and_depth": (None, [vp, vp, vp, vp, vp, i32, u32]),
        "refk_linear_transformer": (None, [u32, f64, f64, vp, vp]),
        "refk_matrix_multiply_1x1n": (None, [f32, u32, vp]),
        "refk_decompose_network_in_and_out": (None, [vp, vp, vp, u32, u32]),
        "refk_init_xyzs": (None, [vp, u32, u32]),
        "refk_dd_scale": (None, [vp, vp, u32, u32, f32, f32]),
        "refk_add_random": (None, [vp, u32, u32, u32, f32, f32]),
        "refk_dg_update": (None, [vp, vp, f32, u32, u32]),
        "refk_srgb_to_linear": (None, [vp, vp, u32]),
        "refk_linear_to_srgb": (None, [vp, vp, u32]),
        "refk_pcg32_first_float": (f32, [C.c_uint64, C.c_uint64]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    assert L.refk_ngpu() == 2, "the driver below restates the NGPU = 2 loop"
    _lib = L
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return a.ctypes.data


def div_round_up(a, b):
    return (a + b - 1) // b


class Geometry:
    """What the march takes from a model (nerf_render.cu:305-309): a ModelDesc's scalars and its density grid."""

    def __init__(self, desc):
        self.bound, self.scale, self.mean_density = float(desc.bound), float(desc.scale), float(desc.mean_density)
        self.cascade, self.H = int(desc.cascade), int(desc.density_grid_size)
        self.aabb = np.array(list(desc.aabb), np.float32)
        self.grid = np.ctypeslib.as_array(desc.density_grid, shape=(int(desc.n_density_grid),)).astype(np.float32).copy()
        assert self.grid.size == self.cascade * self.H ** 3


# ------------------------------------------------------------------------------------------------------------ single kernels
def nerf_matrix_to_ngp(pose, scale):
    pose, out = _f32(pose).reshape(16), np.empty(16, np.float32)
    lib().refk_nerf_matrix_to_ngp(_p(pose), scale, _p(out))
    return out.reshape(4, 4)


def generate_rays_half(cam, pose, scale, W, N, gpuid):
    """set_rays_o + set_rays_d of one device: planar ([3][N], [3][N])"""
    cam, pose = _f32(cam).reshape(4), _f32(pose).reshape(16)
    o, d = np.zeros((3, N), np.float32), np.zeros((3, N), np.float32)
    lib().refk_generate_rays(_p(cam), _p(pose), scale, W, N, gpuid, _p(o), _p(d))
    return o, d


def near_far(rays_o, rays_d, aabb, min_near):
    """kernel_near_far_from_aabb on planar rays [3][N]"""
    rays_o, rays_d, aabb = _f32(rays_o), _f32(rays_d), _f32(aabb).copy()
    N = rays_o.shape[1]
    nears, fars = np.zeros(N, np.float32), np.zeros(N, np.float32)
    lib().refk_near_far_from_aabb(_p(rays_o), _p(rays_d), _p(aabb), N, min_near, _p(nears), _p(fars))
    return nears, fars


def halves(cam, pose, geo, W, H, min_near):
    """Both devices' rays of a W x H frame: [(rays_o, rays_d, nears, fars)] * 2, planar"""
    assert (W * H) % 2 == 0
    N = W * H // 2
    out = []
    for gpu in range(2):
        o, d = generate_rays_half(cam, pose, geo.scale, W, N, gpu)
        out.append((o, d) + near_far(o, d, geo.aabb, min_near))
    return out


def interleave(parts):
    """per-device arrays [..., N] -> pixel order [..., 2N] (pixel = 2 * tid + gpuid)"""
    a, b = parts
    out = np.empty(a.shape[:-1] + (2 * a.shape[-1],), a.dtype)
    out[..., 0::2], out[..., 1::2] = a, b
    return out


def frame_rays(cam, pose, geo, W, H, min_near):
    """The whole frame's rays in pixel order: rays_o [n][3], rays_d [n][3], nears [n], fars [n]"""
    h = halves(cam, pose, geo, W, H, min_near)
    o, d = interleave([h[0][0], h[1][0]]), interleave([h[0][1], h[1][1]])
    return np.ascontiguousarray(o.T), np.ascontiguousarray(d.T), interleave([h[0][2], h[1][2]]), interleave([h[0][3], h[1][3]])


def march(geo, rays_o, rays_d, nears, fars, rays_alive, rays_t, n_alive, n_step, dt_gamma, perturb, i, xyzs=None, dirs=None, deltas=None):
    """kernel_march_rays.  rays_o / rays_d planar [3][N].  The three outputs are PRE-ZEROED here unless given: the reference leaves
    slots it does not write untouched, the project defines them as zero."""
    N = rays_o.shape[1]
    cap = div_round_up(max(n_alive * n_step, 1), THREADS) * THREADS
    xyzs = np.zeros((cap, 3), np.float32) if xyzs is None else xyzs
    dirs = np.zeros((cap, 3), np.float32) if dirs is None else dirs
    deltas = np.zeros((cap, 2), np.float32) if deltas is None else deltas
    lib().refk_march_rays(n_alive, n_step, _p(rays_alive), _p(rays_t), N, _p(rays_o), _p(rays_d), geo.bound, dt_gamma, geo.cascade,
                          geo.H, _p(geo.grid), geo.mean_density, _p(nears), _p(fars), _p(xyzs), _p(dirs), _p(deltas), perturb, i)
    return xyzs, dirs, deltas


def march_first_round(geo, rays_o_n3, rays_d_n3, nears, fars, n_step, dt_gamma, perturb=0):
    """The march of the loop's first round on rays in any order ([n][3] in, rays_alive the identity, rays_t = nears): the stage
    call nrf_march / Oracle.march restates.  Returns xyzs [n][n_step][3], dirs, deltas [n][n_step][2]."""
    n = len(nears)
    o, d = np.ascontiguousarray(_f32(rays_o_n3).T), np.ascontiguousarray(_f32(rays_d_n3).T)
    nears, fars = _f32(nears), _f32(fars)
    alive, t = np.zeros((2, n), np.int32), np.zeros((2, n), np.float32)
    lib().refk_init_step0(_p(alive), _p(t), n, n, _p(nears))
    x, dr, dl = march(geo, o, d, nears, fars, alive, t, n, n_step, dt_gamma, perturb, 0)
    k = n * n_step
    return x[:k].reshape(n, n_step, 3), dr[:k].reshape(n, n_step, 3), dl[:k].reshape(n, n_step, 2)


def composite(sigmas, rgbs, deltas, rays_t, state):
    """kernel_composite_rays on n rays with n_step slots each, in oracle_py.composite's form: sigmas [n][n_step], rgbs
    [n][n_step][3], deltas [n][n_step][2], rays_t [n], state [n][5] = (weights_sum, depth, r, g, b).  Returns (rays_t, state)."""
    sigmas, rgbs, deltas = _f32(sigmas), _f32(rgbs), _f32(deltas)
    n, n_step = sigmas.shape
    cap = n * n_step
    alive, t = np.zeros((2, n), np.int32), np.zeros((2, n), np.float32)
    alive[0], t[0] = np.arange(n), _f32(rays_t)
    state = _f32(state)
    ws, depth, image = state[:, 0].copy(), state[:, 1].copy(), np.ascontiguousarray(state[:, 2:5])
    sig, rgb, dl = sigmas.reshape(cap).copy(), rgbs.reshape(cap, 3).copy(), deltas.reshape(cap, 2).copy()
    lib().refk_composite_rays(n, n_step, _p(alive), _p(t), n, _p(sig), _p(rgb), _p(dl), cap, _p(ws), _p(depth), _p(image), 0)
    return t[0].copy(), np.concatenate([ws[:, None], depth[:, None], image], axis=1)


def linear_transformer(weight, bias, values):
    values = _f32(values)
    out = np.empty_like(values)
    lib().refk_linear_transformer(values.size, float(weight), float(bias), _p(values), _p(out))
    return out


def normalise(bound, xyz, dirs):
    """The two affine maps ahead of the network with the call site's own arguments (nerf_render.cu:311-314)"""
    return linear_transformer(1.0 / (2 * bound), 0.5, xyz), linear_transformer(0.5, 0.5, dirs)


def matrix_multiply_1x1n(a, values):
    values = _f32(values).copy()
    lib().refk_matrix_multiply_1x1n(a, values.size, _p(values))
    return values


def decompose(network_output_u16, n):
    """decompose_network_in_and_out: fp16 bits [rows][cap] -> (sigmas [n], rgbs [n][3])"""
    out = np.ascontiguousarray(network_output_u16, np.uint16)
    cap = out.shape[1]
    sig, rgb = np.zeros(cap, np.float32), np.zeros((cap, 3), np.float32)
    lib().refk_decompose_network_in_and_out(_p(sig), _p(rgb), _p(out), cap, n)
    return sig[:n], rgb[:n]


def get_image_and_depth(image, depth, nears, fars, weights_sum, bg_color):
    image, depth = _f32(image).copy(), _f32(depth).copy()
    nears, fars, weights_sum = _f32(nears), _f32(fars), _f32(weights_sum)
    lib().refk_get_image_and_depth(_p(image), _p(depth), _p(nears), _p(fars), _p(weights_sum), int(bg_color), len(depth))
    return image, depth


def init_xyzs(H):
    dd = np.zeros(3 * H ** 3, np.float32)
    lib().refk_init_xyzs(_p(dd), dd.size, H)
    return dd


def dd_scale(src, dst, H, k, b=0.0):
    src, dst = _f32(src), _f32(dst).copy()
    lib().refk_dd_scale(_p(src), _p(dst), dst.size, H, k, b)
    return dst


def add_random(dd, seed, H, k, b=0.0):
    dd = _f32(dd).copy()
    lib().refk_add_random(_p(dd), seed, dd.size, H, k, b)
    return dd


def dg_update(dg, tmp, decay, H):
    dg, tmp = _f32(dg).copy(), _f32(tmp).copy()
    lib().refk_dg_update(_p(dg), _p(tmp), decay, dg.size, H)
    return dg


def srgb_to_linear(x):
    x = _f32(x)
    out = np.empty_like(x)
    lib().refk_srgb_to_linear(_p(x), _p(out), x.size)
    return out


def linear_to_srgb(x):
    x = _f32(x)
    out = np.empty_like(x)
    lib().refk_linear_to_srgb(_p(x), _p(out), x.size)
    return out


def to_u8(x):
    """`(unsigned char)(255.0 * x)` of nerf_render.cu:355-358 (host code inside render_frame, restated): the float promotes to
    double, the product truncates toward zero.  The conversion is defined only for products in (-1, 256) (SURVEY.md Appendix
    D-2: outside it the reference's behaviour is undefined, the project saturates): returns (bytes, defined mask)."""
    p = 255.0 * np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        defined = (p > -1) & (p < 256)
    return np.trunc(np.where(defined, p, 0)).astype(np.uint8), defined


# ------------------------------------------------------------------------------------------------------------ render_frame
def network_through_reference_maps(oracle, geo, xyzs, dirs, density_scale=1.0):
    """The network leg of one round (nerf_render.cu:311-329) on m live samples: the reference's two linear_transformer calls, the
    ORACLE's encodings and MLPs on their output (the reference's are tiny-cuda-nn's: not built here), the reference's
    decompose_network_in_and_out on the fp16 result and, when density_scale != 1, its matrix_multiply_1x1n."""
    m = len(xyzs)
    p01, d01 = normalise(geo.bound, xyzs, dirs)
    out4 = oracle.mlp_forward(oracle.encode_grid(p01), oracle.encode_dir(d01))  # fp16 bits [m][4] = r, g, b, sigma
    cap = div_round_up(max(m, 1), THREADS) * THREADS
    net = np.zeros((16, cap), np.uint16)  # padded_output_width rows; rows 0-2 colour, row 3 density (render_utils.h:326-331)
    net[:4, :m] = out4.T
    sig, rgb = decompose(net, m)
    if density_scale != 1:
        sig = matrix_multiply_1x1n(density_scale, sig)
    return sig, rgb


def render_loop(oracle, geo, rays_o, rays_d, nears, fars, opts, log=None):
    """The loop of render_frame for ONE device's N rays (nerf_render.cu:261-343), every kernel the reference's, the network leg as
    above.  Two things follow the project's stated decisions and not the literal reference, both needed for a defined result:
    `deltas` is zeroed ahead of every march (Appendix D-1: the reference composites whatever an earlier round left in unwritten
    slots) and only written slots go through the network (D-5: their outputs are never composited, the `deltas == 0` exit
    comes first).  Returns (image [N][3], depth [N], weights_sum [N]) after get_image_and_depth."""
    L = lib()
    N = len(nears)
    ws, depth, image = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros((N, 3), np.float32)  # :262-267
    alive, rays_t = np.zeros((2, N), np.int32), np.zeros((2, N), np.float32)
    step, i, num_alive = 0, 0, N
    while True:
        if step >= opts.max_steps:  # :270
            break
        if step == 0:
            L.refk_init_step0(_p(alive), _p(rays_t), N, num_alive, _p(nears))
        else:
            new_i, old_i = i % 2, (i + 1) % 2  # :286-290
            num_alive = L.refk_compact_rays(num_alive, _p(alive), _p(rays_t), N, new_i, old_i)
        if num_alive <= 0:  # :294
            break
        num_step = max(min(N // num_alive, 8), 1)  # :300
        if log is not None:
            log.append((num_alive, num_step))
        xyzs, dirs, deltas = march(geo, rays_o, rays_d, nears, fars, alive, rays_t, num_alive, num_step, opts.dt_gamma,
                                   1 if opts.perturb else 0, i)
        cap = len(deltas)  # step_x_alive, :302
        sig, rgb = np.zeros(cap, np.float32), np.zeros((cap, 3), np.float32)
        live = np.flatnonzero(deltas[:, 0] != 0)
        if len(live):
            sig[live], rgb[live] = network_through_reference_maps(oracle, geo, xyzs[live], dirs[live], opts.density_scale)
        L.refk_composite_rays(num_alive, num_step, _p(alive), _p(rays_t), N, _p(sig), _p(rgb), _p(deltas), cap, _p(ws), _p(depth),
                              _p(image), i)
        step += num_step  # :336
        i += 1
    bg = int(opts.bg_color)
    assert bg == opts.bg_color, "the reference's background is an int (nerf_render.h:74)"
    L.refk_get_image_and_depth(_p(image), _p(depth), _p(nears), _p(fars), _p(ws), bg, N)
    return image, depth, ws


def render_frame(oracle, geo, cam, pose, W, H, opts, one_device=False, log=None):
    """render_frame (nerf_render.cu:238-360) up to the float planes: rgb [H][W][3], depth [H][W], alpha [H][W], nears [H][W].
    one_device = False: the two halves of the NGPU = 2 build, each through its own loop (its step rule sees N = W * H / 2).
    one_device = True: the same kernels with the whole frame in ONE loop (N = W * H) -- the single-device program the two-device
    one was made from, and the loop the oracle's SCHED_REFERENCE restates."""
    h = halves(cam, pose, geo, W, H, opts.min_near)
    if one_device:
        o, d = interleave([h[0][0], h[1][0]]), interleave([h[0][1], h[1][1]])
        nr, fr = interleave([h[0][2], h[1][2]]), interleave([h[0][3], h[1][3]])
        image, depth, ws = render_loop(oracle, geo, np.ascontiguousarray(o), np.ascontiguousarray(d), nr, fr, opts, log)
    else:
        parts = [render_loop(oracle, geo, *h[g], opts, None if log is None else log.setdefault(g, [])) for g in range(2)]
        image = interleave([parts[0][0].T, parts[1][0].T]).T
        depth, ws = interleave([parts[0][1], parts[1][1]]), interleave([parts[0][2], parts[1][2]])
        nr = interleave([h[0][2], h[1][2]])
    return image.reshape(H, W, 3), depth.reshape(H, W), ws.reshape(H, W), nr.reshape(H, W)


# ------------------------------------------------------------------------------------------------- the encoding kernels
# oracle/_ref/libref_encodings.so (oracle/ref_encodings.cpp): tiny-cuda-nn's kernel_grid + transpose_encoded_position, kernel_sh,
# frequency_encoding, identity, warp_activation and the GridEncodingTemplated constructor.  T = the reference's tiny-cuda-nn.
ENC_LIB = ROOT / "oracle" / "_ref" / "libref_encodings.so"
TCNN = REFERENCE / "dependencies" / "tiny-cuda-nn" / "include" / "tiny-cuda-nn"
_enc = None


def require_encodings():
    """As require(), for the encoding library."""
    import pytest

    if not ENC_LIB.exists():
        if reference_tree_exists():
            pytest.fail(f"{ENC_LIB} is missing although the reference tree {REFERENCE} exists: run `make -C oracle ref` (build() does)")
        pytest.skip("no reference tree and no oracle/_ref/libref_encodings.so: nothing to hold the oracle's encodings to on this machine")
    return enc_lib()


def enc_lib():
    global _enc
    if _enc is not None:
        return _enc
    L = C.CDLL(str(ENC_LIB))
    vp, u32, i32, f32 = C.c_void_p, C.c_uint32, C.c_int, C.c_float
    sig = {
        "refk_enum_value": (i32, [C.c_char_p]),
        "refk_grid_encode": (i32, [u32, u32, u32, vp, u32, f32, i32, i32, vp, vp, vp, u32]),
        "refk_grid_table": (i32, [u32, u32, u32, u32, f32, i32, vp, vp, vp]),
        "refk_grid_index": (i32, [u32, i32, u32, u32, u32, vp, vp]),
        "refk_fast_hash3": (None, [u32, vp, vp]),
        "refk_sh": (None, [u32, u32, u32, vp, vp]),
        "refk_frequency": (None, [u32, u32, u32, vp, vp]),
        "refk_identity": (None, [u32, u32, f32, f32, vp, vp]),
        "refk_activation": (None, [i32, u32, vp, vp]),
        "refk_half_add": (None, [u32, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _enc = L
    return L


def enum_value(name):
    v = enc_lib().refk_enum_value(name.encode())
    assert v >= 0, name
    return v


# nerfhip.h's numbering (NRF_GRID_*, NRF_INTERP_*, NRF_ACT_*) -> the reference's enumerator
GRID_TYPES = {0: "GridType::Hash", 1: "GridType::Dense", 2: "GridType::Tiled"}
INTERPOLATIONS = {0: "InterpolationType::Linear", 1: "InterpolationType::Nearest", 2: "InterpolationType::Smoothstep"}
ACTIVATIONS = {0: "Activation::None", 1: "Activation::ReLU", 2: "Activation::Exponential", 3: "Activation::Sigmoid",
               4: "Activation::Squareplus", 5: "Activation::Softplus", 6: "Activation::Sine"}


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _u16(a):
    return np.ascontiguousarray(a, dtype=np.uint16)


def grid_table(F, n_levels, log2_hashmap_size, base_resolution, per_level_scale, grid_type):
    """The GridEncodingTemplated<__half, 3, F> constructor (grid.h:875-940): (offsets [L + 1], resolutions [L], n_params), or None
    where it throws.  grid_type is nerfhip.h's number."""
    offsets, res, n_params = np.zeros(n_levels + 1, np.uint32), np.zeros(n_levels, np.uint32), C.c_uint64()
    rc = enc_lib().refk_grid_table(F, F * n_levels, log2_hashmap_size, base_resolution, per_level_scale, enum_value(GRID_TYPES[grid_type]),
                                   _p(offsets), _p(res), C.addressof(n_params))
    assert rc in (0, 1), f"refk_grid_table: {rc} (the constructor's report could not be read)"
    return None if rc else (offsets, res, int(n_params.value))


def grid_encode(desc, offsets, table_f16, pos01, padded):
    """kernel_grid<__half, 3, F> + transpose_encoded_position as GridEncodingTemplated::forward_impl launches them (grid.h:942-1018):
    uint16 [n][padded].  desc: a ModelDesc; offsets: the level offsets; table_f16: the grid's parameters as fp16 bits."""
    pos01, offsets, table_f16 = _f32(pos01).reshape(-1, 3), _u32(offsets), _u16(table_f16)
    F, L = int(desc.n_features_per_level), int(desc.n_levels)
    assert len(offsets) == L + 1 and len(table_f16) == int(offsets[L]) * F
    out = np.full((len(pos01), padded), 0xDEAD, np.uint16)
    rc = enc_lib().refk_grid_encode(F, len(pos01), F * L, _p(offsets), int(desc.base_resolution), float(desc.per_level_scale),
                                    enum_value(INTERPOLATIONS[int(desc.interpolation)]), enum_value(GRID_TYPES[int(desc.grid_type)]),
                                    _p(table_f16), _p(pos01), _p(out), padded)
    assert rc == 0
    return out


def grid_index(F, grid_type, hashmap_size, resolution, corners):
    """grid_index<3, F>(.., feature 0, ..) (grid.h:100-117) over corners uint32 [n][3]: F * entry"""
    corners = _u32(corners).reshape(-1, 3)
    out = np.empty(len(corners), np.uint32)
    assert enc_lib().refk_grid_index(F, enum_value(GRID_TYPES[grid_type]), int(hashmap_size), int(resolution), len(corners), _p(corners), _p(out)) == 0
    return out


def fast_hash3(corners):
    corners = _u32(corners).reshape(-1, 3)
    out = np.empty(len(corners), np.uint32)
    enc_lib().refk_fast_hash3(len(corners), _p(corners), _p(out))
    return out


def encode_dir(kind, arg, dir01, padded):
    """kernel_sh (kind 0, arg = degree), frequency_encoding (1, n_frequencies) or identity (2) as their encodings' forward_impl
    launch them, with the padding that brings the row to `padded`: uint16 [n][padded]"""
    dir01 = _f32(dir01).reshape(-1, 3)
    raw = {0: arg * arg, 1: 6 * arg, 2: 3}[kind]
    out = np.full((len(dir01), padded), 0xDEAD, np.uint16)
    L = enc_lib()
    if kind == 0:
        L.refk_sh(len(dir01), arg, padded - raw, _p(dir01), _p(out))
    elif kind == 1:
        L.refk_frequency(len(dir01), arg, padded - raw, _p(dir01), _p(out))
    else:
        L.refk_identity(len(dir01), padded - raw, 1.0, 0.0, _p(dir01), _p(out))
    return out


def activation(act, bits):
    """warp_activation<__half> (common_device.h:68-114) of fp16 bit patterns; act is nerfhip.h's number"""
    bits = _u16(bits)
    out = np.empty_like(bits)
    enc_lib().refk_activation(enum_value(ACTIVATIONS[act]), bits.size, _p(bits), _p(out))
    return out


def half_add(a, b):
    a, b = _u16(a), _u16(b)
    out = np.empty_like(a)
    enc_lib().refk_half_add(a.size, _p(a), _p(b), _p(out))
    return out
