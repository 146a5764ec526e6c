"""The stage kernels and the pixel-format kernels of csrc/nrf_kernels.hip past one pass of their capped grids.

Every one of them walks its rows in a grid-stride loop; the older tests call them with fewer rows than one pass of the grid consumes,
so that no line carried from one trip of the loop to the next -- a counter's step, mlp_forward_kernel's rotation of three row buffers
and its prefetch two chunks ahead, the exits of its form unrolled by three -- ran under a test that looks at values.  Here every
kernel runs at sizes relative to P, its pass, which the tests take from host/stage_plan_check.cpp (tests/stage_plan_rows.py: the text
the launchers compile), never from a literal: 1, P - 1, P, P + 1, 2 P + 17 and what the sections add.

Every output buffer is filled beforehand with a pattern no result can equal -- a NaN with a payload for fp16 and fp32, two runs with
complementary bytes for byte outputs -- and carries 64 guard rows past n: every row below n must have been written, every guard row
left bit-identical.  The expectations are the float64 chain of the dense probe models (tests/dense_reference.py) for the MLP stage and
the CPU oracle for everything else, at the tolerances the older tests of the same entry points state (bit-exact where they are).

mlp_forward_kernel's forms 20 and 21 are chosen by NRF_MLP_FORM, which the library reads once per process: they run the same check in
a fresh child process each (this file run as a program), one after the other."""
if __name__ == "__main__":
    import sys
    from pathlib import Path

    _root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(_root / "nerf-cuda_amd"), str(_root / "tests"), str(_root)]

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # (before anything loads libnerfhip.so: the two then share torch's HIP runtime)
pytestmark = pytest.mark.gpu

import dense_model as dm  # noqa: E402
import dense_reference as dr  # noqa: E402
import grid_plan_rows as gpr  # noqa: E402
import model_image_rows as mir  # noqa: E402
import models  # noqa: E402
import nerfhip as nh  # noqa: E402
import oracle_py as op  # noqa: E402
import probe_model as pm  # noqa: E402
import stage_plan_rows as spr  # noqa: E402
import synthetic as syn  # noqa: E402
from test_dense_gpu import _as_device_halves, _crafted_inputs  # noqa: E402
from test_probe_gpu import _context, _plan  # noqa: E402

GUARD = 64             # guard rows past n in every output buffer
NAN16 = 0x7E5A         # an fp16 NaN with a payload: no kernel here produces it (a computed NaN is the canonical 0x7e00 / 0xfe00)
NAN32 = 0x7FC5A5A5     # ... and its fp32 counterpart
FILLS8 = (0xA5, 0x5A)  # byte outputs: every byte is a possible result, so two runs with complementary fills
BASE = 4099            # rows of the MLP stage's base set: prime, so no pass is a multiple of it


def sync():
    torch.cuda.synchronize()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _common(P):
    return [1, P - 1, P, P + 1, 2 * P + 17]


def _half(k, P):
    """floor(k P / 2) + 17: waves make floor(k / 2) + 1 and floor(k / 2) trips for odd k"""
    return k * P // 2 + 17


def _filled16(rows, cols):
    return torch.full((rows + GUARD, cols), NAN16, dtype=torch.int16, device="cuda")


def _filled32(rows, cols):
    return torch.full((rows + GUARD, cols), NAN32, dtype=torch.int32, device="cuda")


def _filled8(n_bytes, guard_bytes, fill):
    return torch.full((n_bytes + guard_bytes,), fill, dtype=torch.uint8, device="cuda")


def _written(buf, n, pattern, what):
    """the first n rows of an output buffer as an unsigned array: none of their elements still holds the fill, every guard row does"""
    a = buf.cpu().numpy()
    a = a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])
    assert len(a) == n + GUARD
    assert np.all(a[n:] == pattern), (what, "a guard row was written", np.flatnonzero((a[n:] != pattern).reshape(GUARD, -1).any(axis=1))[:8].tolist())
    stale = (a[:n] == pattern).reshape(n, -1).any(axis=1)
    assert not stale.any(), (what, f"{int(stale.sum())} rows below n were not written, the first: {np.flatnonzero(stale)[:8].tolist()}")
    return a[:n]


def _trips(kind, sizes):
    return {r.n: (r.trips_first, r.trips_last) for r in spr.rows([(kind, n) for n in sizes])}


# --------------------------------------------------------------------------- a, b: nrf_mlp_forward
def check_mlp_trips(name, form, log=print):
    """nrf_mlp_forward with the dense probe model of pm.INSTANCES[name] on rows every one of which dense_reference.chain certifies: row i
    of a call is row i % BASE of the base set, the expectation the float64 chain's row i % BASE.  rgb array_equal, sigma ==
    fp16(exp(g0)) to rtol 2e-3 (v_exp_f32, tests/test_dense_gpu.py), nrf_mlp_forward_repeat(3) the same bits.  form: the hot stage's
    NRF_MLP_FORM in force in this process (None: the model goes through the generic stage)."""
    kw, own, stage, env = pm.INSTANCES[name]
    desc, keep, info = dm.dense_desc(dict(pm.T12, **kw), dm.SEEDS_OF.get(name, dm.SEEDS)[0], None)
    assert _plan(desc, int(env.get("NRF_WIDTH_INSTANCES", "1")), 8192)[1] == stage
    hot = stage == pm.HOT
    assert hot == (form is not None)
    kind = f"mlp_forward:{form}" if hot else "gen_mlp_forward"
    P = spr.one_pass(kind)
    if hot:  # {1, 2}, {2, 3}, {3, 4}, {4, 5} trips: every exit of the loop unrolled by three, one full turn of the buffer roles
        sizes = _common(P) + [_half(k, P) for k in (3, 5, 7, 9)]
        expect = {_half(3, P): (2, 1), _half(5, P): (3, 2), _half(7, P): (4, 3), _half(9, P): (5, 4), P: (1, 1), P + 1: (2, 1)}
    else:
        sizes = [P - 1, P + 1, 2 * P + 17, _half(7, P)]
        expect = {P - 1: (1, 1), P + 1: (2, 1), _half(7, P): (4, 3)}
    repeat_at = _half(7, P)
    got_trips = _trips(kind, sizes)
    for n, t in expect.items():
        assert got_trips[n] == t, (kind, n, got_trips[n], t)
    assert all(n % 32 for n in sizes if n > P + 1) and P % BASE  # ragged last chunks; no pass is a multiple of the base set

    feat, dirf = _crafted_inputs(info, BASE, 100 + BASE)
    c = dr.chain(info["D"], info["R"], info["act"], feat, dirf)
    assert c["certified"].all() and np.all(np.isfinite(c["rgb"])), name
    want_rgb = np.asarray(c["rgb"])
    want_sigma = np.exp(c["g"][:, 0].astype(np.float32)).astype(np.float16).astype(np.float32)
    assert np.all(np.isfinite(want_sigma))
    # a chunk taken from the buffer of a neighbouring trip changes its rows: rows a whole number of passes apart share no expectation
    i = np.arange(BASE)
    for k in (1, 2, 3, 4):
        same = float((want_rgb[i] == want_rgb[(i + k * P) % BASE]).all(axis=1).mean())
        assert same < 0.01, (name, k, same)

    n_max = max(sizes)
    idx_d = torch.arange(n_max, device="cuda") % BASE
    f_d, d_d = _as_device_halves(feat)[idx_d].contiguous(), _as_device_halves(dirf)[idx_d].contiguous()
    ctx = _context(env)
    try:
        ctx.load_model(desc)
        for n in sizes:
            idx = np.arange(n) % BASE
            out = _filled16(n, 4)
            sync()
            ctx.mlp_forward(f_d.data_ptr(), d_d.data_ptr(), n, out.data_ptr())
            sync()
            bits = _written(out, n, NAN16, (name, kind, n))
            got = bits.view(np.float16)
            bad = (got[:, :3].astype(np.float32) != want_rgb[idx]).any(axis=1)
            log(f"{name} {kind} n={n} trips={got_trips[n]} rgb rows that differ: {int(bad.sum())}")
            assert not bad.any(), (name, kind, n, f"{int(bad.sum())} rows differ, the first: {np.flatnonzero(bad)[:8].tolist()}")
            np.testing.assert_allclose(got[:, 3].astype(np.float32), want_sigma[idx], rtol=2e-3)
            if n == repeat_at:
                again = _filled16(n, 4)
                sync()
                ctx.mlp_forward_repeat(f_d.data_ptr(), d_d.data_ptr(), n, again.data_ptr(), 3)
                sync()
                assert np.array_equal(_written(again, n, NAN16, (name, kind, n, "repeat")), bits), (name, kind, "repeat")
    finally:
        ctx.close()


def test_mlp_forward_hot_stage_walks_its_three_buffers():
    """(a) form 30, the default, in this process: up to five trips per wave"""
    assert os.environ.get("NRF_MLP_FORM") in (None, "30")
    check_mlp_trips("hot", 30)


@pytest.mark.parametrize("form", ["20", "21"])
def test_mlp_forward_hot_stage_other_forms_in_a_child_process(form):
    """(a) forms 20 (two workgroups per compute unit, rotation by copies) and 21 (by name: the loop unrolled by three) -- compiled into
    the library, chosen by NRF_MLP_FORM once per process: the same check in a fresh process"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "mlp", "hot", form], env=dict(os.environ, NRF_MLP_FORM=form),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (form, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert f"mlp_forward:{form}" in r.stdout and "done" in r.stdout


@pytest.mark.parametrize("name", ["generic_w32_h2", "wide_freq12"])
def test_mlp_forward_generic_stage_past_one_pass(name):
    """(b) gen_mlp_forward_kernel: a generic model, and a wide one (whose rows go through the generic stage kernel: stage_model)"""
    check_mlp_trips(name, None)


def test_mlp_forward_refuses_misaligned_buffers():
    """feat 16 bytes, dirfeat and out 8 (include/nerfhip.h): anything else is NRF_E_INVALID before a launch -- the outputs stay as they were"""
    desc, keep, cfg = models.build_model(log2_hashmap_size=12, H=32)
    ctx = nh.NerfHip(0)
    try:
        ctx.load_model(desc)
        n = 64
        f_d = torch.zeros((n + 1, 32), dtype=torch.int16, device="cuda")
        d_d = torch.zeros((n + 1, 16), dtype=torch.int16, device="cuda")
        out = _filled16(n, 4)
        sync()
        for what, args in (("feat", (f_d.data_ptr() + 8, d_d.data_ptr(), out.data_ptr())), ("dirfeat", (f_d.data_ptr(), d_d.data_ptr() + 4, out.data_ptr())),
                           ("out", (f_d.data_ptr(), d_d.data_ptr(), out.data_ptr() + 4))):
            for repeat in (1, 3):
                with pytest.raises(nh.NerfHipError) as e:
                    ctx.mlp_forward_repeat(args[0], args[1], n, args[2], repeat)
                assert e.value.code == nh.NRF_E_INVALID, (what, e.value.code)
        sync()
        assert np.all(out.cpu().numpy().view(np.uint16) == NAN16)
        ctx.mlp_forward(f_d.data_ptr(), d_d.data_ptr(), n, out.data_ptr())  # (aligned: accepted)
        sync()
        _written(out, n, NAN16, "aligned")
    finally:
        ctx.close()


# --------------------------------------------------------------------------- c: nrf_encode_grid
EDGE_POS = np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0.5], [0.5, 1, 0], [0.25, 0.5, 0.75], [1 - 2 ** -24, 2 ** -24, 0.5], [0.5, 0.5, 0.5],
                     [1 / 3, 2 / 3, 1.0]], np.float32)  # (test_encode_grid_bit_exact)
# id -> (build_model keywords, gather_copy_budget_mb, lane addresses per sample, fast_interp, kind)
GRID_CASES = {
    "t19-copies-near-and-far": (dict(log2_hashmap_size=19, H=32), 6000, 56, 0, "encode_grid"),
    "t19-no-copies": (dict(log2_hashmap_size=19, H=32), 1, 128, 0, "encode_grid"),
    "t19-fast-interp": (dict(log2_hashmap_size=19, H=32), 256, 80, 1, "encode_grid"),
    "generic-f4-l8": (dict(log2_hashmap_size=12, H=32, n_features_per_level=4, n_levels=8), 1, None, 0, "gen_encode_grid:8"),
}
_GRID_WANT = {}  # the oracle's answer, shared by the cases of a model


def _loaded_plan(ctx):
    """the plan's part of the loaded context's model (nrf_debug_model_readout, part "plan"): stage, quad_mask, quad_far, ..."""
    fn = ctx.lib.nrf_debug_model_readout
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    words, n = np.zeros(len(mir.PLAN_WORDS), np.uint32), C.c_uint64(0)
    rc = fn(ctx.h, mir.PARTS.index("plan"), words.ctypes.data_as(C.c_void_p), words.nbytes, C.byref(n))
    assert rc == nh.NRF_OK and n.value == words.nbytes, (rc, n.value)
    return dict(zip(mir.PLAN_WORDS, (int(v) for v in words)))


@pytest.mark.parametrize("case", list(GRID_CASES))
def test_encode_grid_past_one_pass(case):
    """Bit-exact against op.Oracle.encode_grid: the eight edge positions of test_encode_grid_bit_exact at rows 0..7 and again at rows
    P..P + 7, the rest uniform, sizes up to 3 P + 5.  (The oracle encodes the 98 309 positions of the 2^19 table in 0.4 s and the
    196 613 of the generic grid in 0.1 s on a CPU: every row is compared, nothing is tiled.)  fast_interp keeps its stated tolerance."""
    kw, budget, addrs, fast, kind = GRID_CASES[case]
    desc, keep, cfg = models.build_model(**kw)
    P = spr.one_pass(kind)
    sizes = _common(P) + [3 * P + 5]
    trips = _trips(kind, sizes)
    assert trips[P] == (1, 1) and trips[P + 1] == (2, 1) and trips[3 * P + 5] == (4, 3), trips
    n_max = max(sizes)
    pos = np.random.default_rng(21).random((n_max, 3), dtype=np.float32)
    pos[:8] = EDGE_POS
    pos[P:P + 8] = EDGE_POS
    key = (tuple(sorted(kw.items())), n_max)
    if key not in _GRID_WANT:
        _GRID_WANT.clear()
        _GRID_WANT[key] = op.Oracle(desc).encode_grid(pos)
    want = _GRID_WANT[key]
    width = want.shape[1]
    d = nh.ModelDesc.from_buffer_copy(desc)  # (the pointers stay `keep`'s)
    d.gather_copy_budget_mb = budget
    ctx = nh.NerfHip(0)
    try:
        ctx.load_model(d)
        plan = _loaded_plan(ctx)
        if kind == "encode_grid":  # the copies the loaded model reads: two lane addresses for a level with a quad copy, eight without
            assert plan["stage"] == pm.HOT and sum(2 if (plan["quad_mask"] >> lv) & 1 else 8 for lv in range(16)) == addrs, (case, plan)
            assert (plan["quad_mask"] != 0) == (addrs < 128) and (plan["quad_far"] != 0) == (addrs == 56), (case, plan)
        else:
            assert plan["stage"] == pm.GENERIC
        if fast:
            opts = nh.default_options()
            opts.fast_interp = 1
            ctx.set_options(opts)
        p_d = dev(pos)
        for n in sizes:
            out = _filled16(n, width)
            sync()
            ctx.encode_grid(p_d.data_ptr(), n, out.data_ptr())
            sync()
            got = _written(out, n, NAN16, (case, n))
            if not fast:
                bad = (got != want[:n]).any(axis=1)
                assert not bad.any(), (case, n, f"{int(bad.sum())} rows differ, the first: {np.flatnonzero(bad)[:8].tolist()}")
            else:  # its stated tolerance (test_fast_interp_is_opt_in_and_within_its_stated_tolerance) against the exact path, which is the oracle's
                a, b = want[:n].view(np.float16).astype(np.float32), got.view(np.float16).astype(np.float32)
                err = np.abs(a - b)
                assert err.max() <= 4 * 2.0 ** -11, (case, n, float(err.max()))
                if n >= P - 1:
                    assert np.percentile(err, 99.9) <= 2.0 ** -11 and (a != b).any()
    finally:
        ctx.close()


# --------------------------------------------------------------------------- d: nrf_encode_dir
@pytest.mark.parametrize("sh_degree,kind,stage", [(4, "encode_dir", pm.HOT), (8, "gen_encode_dir", pm.GENERIC)])
def test_encode_dir_past_one_pass(sh_degree, kind, stage):
    desc, keep, cfg = models.build_model(log2_hashmap_size=12, H=32, sh_degree=sh_degree)
    assert _plan(desc, 1, 8192)[1] == stage
    P = spr.one_pass(kind)
    sizes = [P - 1, P + 1, 2 * P + 17]
    trips = _trips(kind, sizes)
    assert trips[P - 1] == (1, 0) and trips[P + 1] == (2, 1) and trips[2 * P + 17] == (3, 2), trips
    d = np.random.default_rng(22).normal(size=(max(sizes), 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d01 = (d * np.float32(0.5) + np.float32(0.5)).astype(np.float32)
    want = op.Oracle(desc).encode_dir(d01)
    ctx = nh.NerfHip(0)
    try:
        ctx.load_model(desc)
        d_d = dev(d01)
        for n in sizes:
            out = _filled16(n, want.shape[1])
            sync()
            ctx.encode_dir(d_d.data_ptr(), n, out.data_ptr())
            sync()
            got = _written(out, n, NAN16, (kind, n))
            bad = (got != want[:n]).any(axis=1)
            assert not bad.any(), (kind, n, f"{int(bad.sum())} rows differ, the first: {np.flatnonzero(bad)[:8].tolist()}")
    finally:
        ctx.close()


# --------------------------------------------------------------------------- e, f: nrf_generate_rays, nrf_march, nrf_composite
RAYS_W, RAYS_H = 1024, 513  # one pass of pixels and 1024 more
RAYS_POSE = syn.orbit_pose(45, 25, radius=1.5)  # nine rays of ten meet occupied space, every ray of the last image row among them


def _ray_buffers():
    n = RAYS_W * RAYS_H
    return _filled32(n, 3), _filled32(n, 3), _filled32(n, 1), _filled32(n, 1)


@pytest.mark.parametrize("W,H", [(RAYS_W, RAYS_H), (1023, 513)])  # (the second: a last block that is not full)
def test_generate_rays_past_one_pass_and_with_null_outputs(W, H):
    desc, keep, cfg = models.build_model(log2_hashmap_size=12, H=32)
    n = W * H
    assert _trips("generate_rays", [n])[n] == (2, 1) and ((W, H) == (RAYS_W, RAYS_H) or n % 256)
    cam, pose = syn.default_camera(W, H), RAYS_POSE
    want = op.Oracle(desc).generate_rays(cam, pose, W, H)
    ctx = nh.NerfHip(0)
    try:
        ctx.load_model(desc)
        ctx.set_resolution(W, H)
        # all four outputs, then each pair of them with the other two NULL
        for keep_out in ((0, 1, 2, 3), (1, 2), (0, 3)):
            bufs = [_filled32(n, 3), _filled32(n, 3), _filled32(n, 1), _filled32(n, 1)]
            sync()
            ctx.generate_rays(cam, pose, *[b.data_ptr() if k in keep_out else 0 for k, b in enumerate(bufs)])
            sync()
            for k, b in enumerate(bufs):
                if k in keep_out:
                    got = _written(b, n, NAN32, ("rays", k, keep_out)).view(np.float32).reshape(want[k].shape)
                    np.testing.assert_array_equal(got, want[k])
                else:
                    assert np.all(b.cpu().numpy().view(np.uint32) == NAN32)
    finally:
        ctx.close()


# geometry (tests/test_reference_kernels_cpu.py GEOMETRIES), perturb, march_kernel<COARSE> (a side that is a multiple of 4 has a coarse level)
MARCH_CASES = [("h32", dict(H=32, bound=1.0, cascade=1), 0, True), ("h32-b4-c3", dict(H=32, bound=4.0, cascade=3), 0, True),
               ("h32", dict(H=32, bound=1.0, cascade=1), 5, True), ("h30", dict(H=30, bound=1.0, cascade=1), 0, False)]


@pytest.mark.parametrize("name,geo,perturb,coarse", MARCH_CASES, ids=[f"{c[0]}-perturb{c[2]}" for c in MARCH_CASES])
def test_march_and_composite_past_one_pass(name, geo, perturb, coarse):
    """The rays of a 1024 x 513 frame, n_step 3: march bit-exact against the oracle, composite at the tolerances of
    test_march_bit_exact_and_composite (2e-5 absolute; the T ~ 1e-4 ties below 1e-3 of the rays)."""
    desc, keep, cfg = models.build_model(log2_hashmap_size=12, **geo)
    o = op.Oracle(desc)
    W, H, n_step = RAYS_W, RAYS_H, 3
    n = W * H
    assert _trips("march", [n])[n] == (2, 1) and _trips("composite", [n])[n] == (2, 1)
    P = spr.one_pass("march")
    assert spr.one_pass("composite") == P and n - P >= 1024
    cam, pose = syn.default_camera(W, H), RAYS_POSE
    opts = nh.default_options()
    opts.perturb = perturb
    ctx = nh.NerfHip(0)
    try:
        ctx.load_model(desc)
        ctx.set_options(opts)
        ctx.set_resolution(W, H)
        assert (gpr.readout(ctx)[0]["coarse_shift"] != 0) == coarse  # which march_kernel<COARSE> the launcher picks
        ro, rd, nr, fr = _ray_buffers()
        sync()
        ctx.generate_rays(cam, pose, ro.data_ptr(), rd.data_ptr(), nr.data_ptr(), fr.data_ptr())
        xyzs, dirs, deltas = _filled32(n, n_step * 3), _filled32(n, n_step * 3), _filled32(n, n_step * 2)
        sync()
        ctx.march(ro.data_ptr(), rd.data_ptr(), nr.data_ptr(), fr.data_ptr(), n, n_step, xyzs.data_ptr(), dirs.data_ptr(), deltas.data_ptr())
        sync()
        host = [_written(b, n, NAN32, "rays").view(np.float32) for b in (ro, rd, nr, fr)]
        wx, wd, wdl = o.march(host[0], host[1], host[2].reshape(-1), host[3].reshape(-1), n_step, opts)
        for what, b, w in (("xyzs", xyzs, wx), ("dirs", dirs, wd), ("deltas", deltas, wdl)):
            got = _written(b, n, NAN32, (name, what)).view(np.float32).reshape(w.shape)
            np.testing.assert_array_equal(got, w, err_msg=what)
        found = wdl[:, :, 0] > 0
        assert found[:P].mean() > 0.5 and found[P:].mean() > 0.5  # samples in the rows of either trip
        # composite on those samples with synthetic sigma / rgb
        rng = np.random.default_rng(4)
        sig = rng.uniform(0, 400, (n, n_step)).astype(np.float32)
        sig[::3] *= np.float32(20)  # (three short steps at sigma < 400 end no ray: every third ray is dense enough to reach T <= 1e-4)
        rgb = rng.random((n, n_step, 3), dtype=np.float32)
        t0 = host[2].reshape(-1)
        wt, wst = op.composite(sig, rgb, wdl, t0, np.zeros((n, 5), np.float32))
        st_d, t_d = _filled32(n, 5), _filled32(n, 1)
        st_d[:n] = 0
        t_d[:n] = dev(t0.view(np.int32)).reshape(n, 1)
        s_d, r_d = dev(sig), dev(rgb)
        sync()
        ctx.composite(s_d.data_ptr(), r_d.data_ptr(), deltas.data_ptr(), n, n_step, t_d.data_ptr(), st_d.data_ptr())
        sync()
        st = st_d.cpu().numpy().view(np.uint32)
        got_t = t_d.cpu().numpy().view(np.uint32)
        assert np.all(st[n:] == NAN32) and np.all(got_t[n:] == NAN32)
        np.testing.assert_allclose(st[:n].view(np.float32), wst, atol=2e-5)
        got_t = got_t[:n].view(np.float32).reshape(-1)
        dead_w, dead_g = wt < 0, got_t < 0
        assert (dead_w != dead_g).mean() < 1e-3  # a T ~ 1e-4 tie may fall either way
        same = ~dead_w & ~dead_g
        np.testing.assert_allclose(got_t[same], wt[same], rtol=1e-6)
        assert dead_w[:P].any() and same[:P].any() and dead_w[P:].any() and same[P:].any()
    finally:
        ctx.close()


# --------------------------------------------------------------------------- g: nrf_quantize_u8, nrf_quantize_rgbd8
SPECIAL_PX = [0.0, 1.0, np.nan, np.inf, -np.inf, 0.5, 1 / 255.0, 254.999 / 255.0]  # (test_quantize_rgbd8_matches_reference_packing)


def test_quantize_past_one_pass():
    P = spr.one_pass("quantize")
    assert spr.one_pass("quantize_rgbd8") == P
    sizes = [1, 255, 256, 257, P - 1, P + 1, 2 * P + 17]
    for kind in ("quantize", "quantize_rgbd8"):
        trips = _trips(kind, sizes)
        assert trips[P - 1] == (1, 0) and trips[P + 1] == (2, 1) and trips[2 * P + 17] == (3, 2), (kind, trips)
    n_max = max(sizes)
    rng = np.random.default_rng(23)
    rgba = rng.uniform(-0.2, 1.2, (n_max, 4)).astype(np.float32)
    depth = rng.uniform(-0.2, 1.2, n_max).astype(np.float32)
    for at in (0, P):
        rgba[at:at + 8, 0] = SPECIAL_PX
        rgba[at:at + 8, 2] = SPECIAL_PX[::-1]
        depth[at:at + 8] = SPECIAL_PX
    rgb8, d8 = op.quantize_u8(rgba, depth)
    rgb8, d8 = rgb8.reshape(n_max, 3), d8.reshape(n_max)
    packed = rgb8[:, 0].astype(np.uint32) | (rgb8[:, 1].astype(np.uint32) << 8) | (rgb8[:, 2].astype(np.uint32) << 16) | (d8.astype(np.uint32) << 24)
    ctx = nh.NerfHip(0)
    try:
        r_d, d_d = dev(rgba), dev(depth)
        for n in sizes:
            for fill in FILLS8:
                o_rgb, o_d, o_p = _filled8(3 * n, 3 * GUARD, fill), _filled8(n, GUARD, fill), _filled8(4 * n, 4 * GUARD, fill)
                sync()
                ctx.quantize_u8(r_d.data_ptr(), d_d.data_ptr(), n, o_rgb.data_ptr(), o_d.data_ptr())
                ctx.quantize_rgbd8(r_d.data_ptr(), d_d.data_ptr(), n, o_p.data_ptr())
                sync()
                g_rgb, g_d, g_p = o_rgb.cpu().numpy(), o_d.cpu().numpy(), o_p.cpu().numpy()
                assert np.all(g_rgb[3 * n:] == fill) and np.all(g_d[n:] == fill) and np.all(g_p[4 * n:] == fill), (n, fill, "a guard row was written")
                np.testing.assert_array_equal(g_rgb[:3 * n].reshape(n, 3), rgb8[:n])
                np.testing.assert_array_equal(g_d[:n], d8[:n])
                np.testing.assert_array_equal(g_p[:4 * n].view(np.uint32), packed[:n])
    finally:
        ctx.close()


# --------------------------------------------------------------------------- h: nrf_untile_views_u8, nrf_untile_views
MARKER = 0xDEADBEEF  # the padding tiles of a shard: never in an output


def _shards(W, H, shards, views, channels, seed):
    """(gathered uint32 [shard][view][tiles_per_shard][64][channels], tiles_per_shard, the views untiled by nh.untile_numpy): random
    words -- NaN bit patterns among them --, the tiles no pixel reads filled with MARKER"""
    tps = nh.tiles_per_shard(W, H, shards)
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 2 ** 32, (shards, views, tps * 64, channels), dtype=np.uint64).astype(np.uint32)
    g[g == MARKER] = 0
    slots = np.arange(shards * tps * 64, dtype=np.int64).reshape(shards, tps * 64, 1)
    read = np.zeros(shards * tps * 64, bool)
    read[nh.untile_numpy(slots, W, H).reshape(-1)] = True
    assert read.sum() == W * H and not read.all()  # partial tiles: there is padding
    g[np.broadcast_to(~read.reshape(shards, 1, tps * 64, 1), g.shape)] = MARKER
    f = g.view(np.float32)
    assert np.isnan(f).sum() > 100
    want = np.stack([nh.untile_numpy(np.ascontiguousarray(g[:, v]), W, H) for v in range(views)])  # [view][H][W][channels]
    assert not (want == MARKER).any()
    return g, tps, want


@pytest.mark.parametrize("W,H,views,shards", [(1924, 1085, 2, 1), (1924, 1085, 2, 3), (1924, 1085, 2, 8), (1001, 700, 1, 1), (1001, 700, 1, 3)])
def test_untile_views_u8_past_one_pass(W, H, views, shards):
    """W % 4 == 0 (and not % 8): a thread per quad of pixels, partial tiles on both axes; else a thread per pixel with byte stores"""
    work = W * H * views // (4 if W % 4 == 0 else 1)
    first, last = _trips("untile_u8", [work])[work]
    assert first >= 2 and W % 8 and H % 8
    g, tps, want = _shards(W, H, shards, views, 1, 30 + shards)
    want = want.reshape(views * H * W)
    want_rgb = np.stack([want & 0xFF, (want >> 8) & 0xFF, (want >> 16) & 0xFF], axis=1).astype(np.uint8)
    want_d = (want >> 24).astype(np.uint8)
    n = views * H * W
    ctx = nh.NerfHip(0)
    try:
        ctx.set_resolution(W, H)
        g_d = dev(g.view(np.int32))
        for fill in FILLS8:
            o_rgb, o_d = _filled8(3 * n, 3 * GUARD, fill), _filled8(n, GUARD, fill)
            sync()
            ctx.untile_views_u8(g_d.data_ptr(), shards, tps, views, o_rgb.data_ptr(), o_d.data_ptr())
            sync()
            g_rgb, g_dp = o_rgb.cpu().numpy(), o_d.cpu().numpy()
            assert np.all(g_rgb[3 * n:] == fill) and np.all(g_dp[n:] == fill), (fill, "a guard row was written")
            np.testing.assert_array_equal(g_rgb[:3 * n].reshape(n, 3), want_rgb)
            np.testing.assert_array_equal(g_dp[:n], want_d)
        # refusals before any launch: shards that are not 16-byte aligned; on the quad path, planes that are not 4-byte aligned
        o_rgb, o_d = _filled8(3 * n, 3 * GUARD, FILLS8[0]), _filled8(n, GUARD, FILLS8[0])
        sync()
        bad = [(g_d.data_ptr() + 4, o_rgb.data_ptr(), o_d.data_ptr())]
        if W % 4 == 0:
            bad += [(g_d.data_ptr(), o_rgb.data_ptr() + 1, o_d.data_ptr()), (g_d.data_ptr(), o_rgb.data_ptr(), o_d.data_ptr() + 2)]
        for a in bad:
            with pytest.raises(nh.NerfHipError) as e:
                ctx.untile_views_u8(a[0], shards, tps, views, a[1], a[2])
            assert e.value.code == nh.NRF_E_INVALID
        sync()
        assert np.all(o_rgb.cpu().numpy() == FILLS8[0]) and np.all(o_d.cpu().numpy() == FILLS8[0])
    finally:
        ctx.close()


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_untile_views_past_one_pass(channels):
    """untile_kernel at 1001 x 700 (more than a pass of pixels), compared on the words: channel counts 1 and 4, and 3, which no other test uses"""
    W, H, views, shards = 1001, 700, 1, 3
    n = W * H * views
    assert _trips("untile", [n])[n] == (2, 1)
    g, tps, want = _shards(W, H, shards, views, channels, 40 + channels)
    ctx = nh.NerfHip(0)
    try:
        ctx.set_resolution(W, H)
        g_d = dev(g.view(np.int32))
        out = _filled32(n, channels)
        sync()
        ctx.untile_views(g_d.data_ptr(), shards, tps, channels, views, out.data_ptr())
        sync()
        got = out.cpu().numpy().view(np.uint32)
        assert np.all(got[n:] == NAN32)
        np.testing.assert_array_equal(got[:n], want.reshape(n, channels))
        assert not (got[:n] == MARKER).any() and not (want == NAN32).any()
    finally:
        ctx.close()


if __name__ == "__main__":
    assert sys.argv[1] == "mlp" and sys.argv[3] == os.environ.get("NRF_MLP_FORM"), sys.argv
    check_mlp_trips(sys.argv[2], int(sys.argv[3]))
    print("done")
