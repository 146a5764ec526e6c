"""The HIP stage entry points against vectors recorded from the REFERENCE's own kernels (tests/golden/reference_kernels.npz).

The fixture was written by tests/golden/make_reference_golden.py from the reference's render_utils.h compiled for the CPU
(oracle/ref_kernels.cpp); tests/test_reference_kernels_cpu.py regenerates it wherever a reference tree exists.  This module
reads the fixture only -- neither the tree nor that library exists on a GPU machine.

Tolerances -- none of them new (tests/test_parity_gpu.py states each):
  * nrf_generate_rays, nrf_march: BIT FOR BIT -- the project's existing claim, now against the reference and not its restatement
  * nrf_composite: v_exp_f32 against expf -> 2e-5 absolute on the state; live rays' t at rtol 1e-6; the dead / alive
    disagreement share below 1e-3 (a T ~ 1e-4 tie may fall either way)
  * nrf_network: to the oracle's MLPs on the reference's normalised inputs at mlp_close, |d| <= 4 * 2^-11 * |x| + 2e-3; the
    hash-grid encoding of those inputs bit for bit

Each case renders the frame's 1 920 rays and compares the fixture's every-16th ray."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

import nerfhip as nh
import oracle_py as op

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
G = np.load(GOLDEN / "reference_kernels.npz")
META = json.loads(bytes(G["meta"]).decode())


def _generator():
    spec = importlib.util.spec_from_file_location("make_reference_golden", GOLDEN / "make_reference_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shapes {got.shape} != {want.shape}"
    diff = got.view(np.uint32) != want.view(np.uint32)
    if diff.any():
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} values differ in their bits; first at {at}: "
                             f"HIP {got[at]!r} reference {want[at]!r}")


def mlp_close(got, want, what):
    """tests/test_parity_gpu.py's MLP tolerance: a few fp16 ulps (fp32 MFMA sums in another order, fp16 after every layer)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    tol = 4 * 2.0 ** -11 * np.abs(want[fin]) + 2e-3
    err = np.abs(got[fin] - want[fin])
    assert np.all(err <= tol), f"{what}: worst {float((err / tol).max()):.2f}x tolerance"


@pytest.fixture(scope="module")
def ctx():
    h = nh.NerfHip(0)
    yield h
    h.close()


def composite_close(ctx, sig, rgb, deltas, t0, state0, want_t, want_state, what):
    n = len(t0)
    st_d, t_d = dev(state0), dev(t0)
    s_d, r_d, d_d = dev(sig), dev(rgb), dev(deltas)
    torch.cuda.synchronize()
    ctx.composite(s_d.data_ptr(), r_d.data_ptr(), d_d.data_ptr(), n, 8, t_d.data_ptr(), st_d.data_ptr())
    np.testing.assert_allclose(st_d.cpu().numpy(), want_state, atol=2e-5, rtol=0, err_msg=what)
    got_t = t_d.cpu().numpy()
    dead_w, dead_g = want_t < 0, got_t < 0
    assert (dead_w != dead_g).mean() < 1e-3, what
    same = ~dead_w & ~dead_g
    np.testing.assert_allclose(got_t[same], want_t[same], rtol=1e-6, err_msg=what)


@pytest.mark.parametrize("name", list(META["geometries"]))
def test_stage_entry_points_against_the_reference_vectors(ctx, name):
    gen = _generator()
    g = {k.split("/", 1)[1]: G[k] for k in G.files if k.startswith(name + "/")}
    W, H, idx = META["W"], META["H"], g["index"]
    assert gen.GEOMETRIES == META["geometries"] and META["log2_hashmap_size"] == 12
    desc, keep = gen.build(name)
    grid = np.ctypeslib.as_array(desc.density_grid, shape=(int(desc.n_density_grid),))
    assert int(gen.grid_hash(grid)) == int(g["grid_hash"].item()), "the model rebuilt here is not the fixture's"
    ctx.load_model(desc)
    opts = nh.default_options()
    assert abs(opts.min_near - META["min_near"]) < 1e-7 and abs(opts.dt_gamma - META["dt_gamma"]) < 1e-9
    ctx.set_options(opts)
    ctx.set_resolution(W, H)
    n = W * H

    # rays, near / far
    ro = torch.empty((n, 3), device="cuda"); rd = torch.empty((n, 3), device="cuda")
    nr = torch.empty(n, device="cuda"); fr = torch.empty(n, device="cuda")
    torch.cuda.synchronize()
    ctx.generate_rays(G["cam"], g["pose"], ro.data_ptr(), rd.data_ptr(), nr.data_ptr(), fr.data_ptr())
    same_bits(ro.cpu().numpy()[idx], g["rays_o"], f"{name} rays_o")
    same_bits(rd.cpu().numpy()[idx], g["rays_d"], f"{name} rays_d")
    same_bits(nr.cpu().numpy()[idx], g["nears"], f"{name} nears")
    same_bits(fr.cpu().numpy()[idx], g["fars"], f"{name} fars")

    # march, first round, the whole frame
    for n_step in (1, 3, 8):
        xyzs = torch.empty((n, n_step, 3), device="cuda"); dirs = torch.empty((n, n_step, 3), device="cuda")
        deltas = torch.empty((n, n_step, 2), device="cuda")
        torch.cuda.synchronize()
        ctx.march(ro.data_ptr(), rd.data_ptr(), nr.data_ptr(), fr.data_ptr(), n, n_step, xyzs.data_ptr(), dirs.data_ptr(),
                  deltas.data_ptr())
        assert (g[f"deltas{n_step}"][..., 0] > 0).sum() >= 8  # (the far views show a small object: few rays emit)
        same_bits(xyzs.cpu().numpy()[idx], g[f"xyzs{n_step}"], f"{name} xyzs n_step {n_step}")
        same_bits(dirs.cpu().numpy()[idx], g[f"dirs{n_step}"], f"{name} dirs n_step {n_step}")
        same_bits(deltas.cpu().numpy()[idx], g[f"deltas{n_step}"], f"{name} deltas n_step {n_step}")

    # compositing: two chained calls; the second starts from the reference's own state so that nothing accumulates
    m = len(idx)
    sig, rgb = gen.composite_inputs(m, 0)
    composite_close(ctx, sig, rgb, g["deltas8"], g["nears"], np.zeros((m, 5), np.float32), g["t1"], g["state1"], f"{name} call 1")
    k2 = g["keep2"]
    assert len(k2) > 0 and (g["t1"] < 0).sum() + (g["t2"] < 0).sum() > 0  # rays handed on, and rays that ended
    o2, d2, t2, f2 = dev(g["rays_o"][k2]), dev(g["rays_d"][k2]), dev(g["t1"][k2]), dev(g["fars"][k2])
    x2 = torch.empty((len(k2), 8, 3), device="cuda"); dr2 = torch.empty((len(k2), 8, 3), device="cuda")
    dl2 = torch.empty((len(k2), 8, 2), device="cuda")
    torch.cuda.synchronize()
    ctx.march(o2.data_ptr(), d2.data_ptr(), t2.data_ptr(), f2.data_ptr(), len(k2), 8, x2.data_ptr(), dr2.data_ptr(), dl2.data_ptr())
    same_bits(dl2.cpu().numpy(), g["deltas2"], f"{name} deltas of the resumed march")
    sig, rgb = gen.composite_inputs(len(k2), 1)
    composite_close(ctx, sig, rgb, g["deltas2"], g["t1"][k2], g["state1"][k2], g["t2"], g["state2"], f"{name} call 2")

    # the network on the march's samples: nrf_network normalises on its own; the reference's linear_transformer output is p01, d01
    live = np.flatnonzero(g["deltas1"][:, 0, 0] != 0)
    xyz, dr = g["xyzs1"][live, 0], g["dirs1"][live, 0]
    p01, d01 = g["p01"][live, 0], g["d01"][live, 0]
    o = op.Oracle(desc)
    feat = o.encode_grid(p01)
    out = torch.empty((len(live), o.feat_width), dtype=torch.int16, device="cuda")
    p_d = dev(p01)
    torch.cuda.synchronize()
    ctx.encode_grid(p_d.data_ptr(), len(live), out.data_ptr())
    assert np.array_equal(out.cpu().numpy().view(np.uint16), feat), f"{name}: hash-grid encoding of the reference's normalised positions"
    want = o.mlp_forward(feat, o.encode_dir(d01)).view(np.float16).astype(np.float32)
    sg = torch.empty(len(live), dtype=torch.float32, device="cuda"); cl = torch.empty((len(live), 3), dtype=torch.float32, device="cuda")
    x_d, d_d = dev(xyz), dev(dr)
    torch.cuda.synchronize()
    ctx.network(x_d.data_ptr(), d_d.data_ptr(), len(live), sg.data_ptr(), cl.data_ptr())
    mlp_close(cl.cpu().numpy(), want[:, :3], f"{name} rgb (network)")
    mlp_close(np.log(sg.cpu().numpy()), np.log(want[:, 3]), f"{name} log sigma (network)")
