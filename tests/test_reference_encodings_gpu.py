"""The HIP encoding entry points against tests/golden/reference_encodings.npz: rows the REFERENCE's own kernels wrote
(tiny-cuda-nn's kernel_grid + transpose_encoded_position, kernel_sh, frequency_encoding, identity compiled for the CPU;
tests/golden/make_reference_encodings_golden.py).  Only the fixture is read: neither a reference tree nor oracle/_ref/ is needed.

  * nrf_encode_grid: bit for bit, for every fixture model nrf_load_model accepts -- the register-resident, wide and generic stage
    instances, whichever the model selects (asserted) -- and, for the reference's configuration, under every gather-copy budget
    of tests/test_parity_gpu.py::test_quad_gather_copies_change_no_bit.  Positions in [0, 1] only.
  * nrf_encode_dir: bit for bit for SphericalHarmonics and Identity; Frequency at the atol = 2e-3 of
    tests/test_parity_gpu.py::test_encode_dir (the device's __sinf against the fixture's libm sinf).
  * nrf_network / nrf_density expose no features: their outputs are held to the oracle's MLPs fed with the FIXTURE's rows, at
    the mlp_close bound of tests/test_reference_kernels_gpu.py.
The fixture's exp2f and sinf are libm's: the grid's level scales are host arithmetic in this library as well (nrf_level_table),
so nothing of the device's exp2f enters the compared rows."""
import ctypes as C
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
G = np.load(GOLDEN / "reference_encodings.npz")
META = json.loads(bytes(G["meta"]).decode())
BUDGETS = (1, 256, 6000)  # MB, passed explicitly: the default depends on the device's free memory


def _generator():
    spec = importlib.util.spec_from_file_location("make_reference_encodings_golden", GOLDEN / "make_reference_encodings_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _generator()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_u16(got, want, what):
    assert got.shape == want.shape, f"{what}: shapes {got.shape} != {want.shape}"
    diff = got != want
    if diff.any():
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} fp16 values differ in their bits; first at {at}: "
                             f"HIP {int(got[at]):#06x} reference {int(want[at]):#06x}")


def mlp_close(got, want, what):
    """tests/test_reference_kernels_gpu.py's MLP tolerance: a few fp16 ulps (fp32 MFMA sums in another order, fp16 after every layer)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    tol = 4 * 2.0 ** -11 * np.abs(want[fin]) + 2e-3
    err = np.abs(got[fin] - want[fin])
    assert np.all(err <= tol), f"{what}: worst {float((err / tol).max()):.2f}x tolerance"


def _rays_instance(ctx):
    fn = ctx.lib.nrf_debug_rays_instance
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
    return int(fn(ctx.h))


def model(name):
    """(desc, keepalive) rebuilt from the fixture's keywords; the table's hash tells a drifting generator from a wrong kernel"""
    desc, keep = gen.build(name)
    if name in META["grid"]:
        info = META["grid"][name]
        assert gen.GRID_MODELS[name] == info["kw"], f"{name}: the fixture was made for other keywords"
        table = gen.table_f16(desc, keep, np.array(info["offsets"], np.uint32))
        assert f"{op.fnv1a(table):016x}" == info["table_fnv1a"], f"{name}: the model generator no longer makes the fixture's table"
    return desc, keep


def load(ctx, name, desc):
    """True when nrf_load_model accepts the model.  A refusal must be the level table's own, for the same reason
    (tests/test_reference_encodings_cpu.py holds nrf_level_table_compute's refusals to the reference's constructor); any other refusal
    of a fixture model is a finding and fails."""
    try:
        ctx.load_model(desc)
        return True
    except nh.NerfHipError as refused:
        with pytest.raises(nh.NerfHipError) as table:
            nh.level_table(desc)
        assert str(table.value) == str(refused), f"{name}: refused for another reason than its level table"
        return False


def encode_grid(ctx, pos, width):
    out = torch.empty((len(pos), width), dtype=torch.int16, device="cuda")
    p_d = dev(pos)
    torch.cuda.synchronize()
    ctx.encode_grid(p_d.data_ptr(), len(pos), out.data_ptr())
    return out.cpu().numpy().view(np.uint16)


def encode_dir(ctx, d01, width):
    out = torch.empty((len(d01), width), dtype=torch.int16, device="cuda")
    d_d = dev(d01)
    torch.cuda.synchronize()
    ctx.encode_dir(d_d.data_ptr(), len(d01), out.data_ptr())
    return out.cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def ctx():
    h = nh.NerfHip(0)
    yield h
    h.close()


def test_the_fixture_reaches_every_stage_instance():
    assert {m["stage"] for m in META["grid"].values()} == {0, 1, 2}  # register-resident, generic, wide
    assert G["pos"].shape == (264, 3) and G["pos"].min() == 0 and G["pos"].max() == 1


@pytest.mark.parametrize("name", list(META["grid"]))
def test_encode_grid_bit_exact_against_kernel_grid(ctx, name):
    desc, keep = model(name)
    if not load(ctx, name, desc):
        return
    stage = META["grid"][name]["stage"]
    assert _rays_instance(ctx) in ((0, 16) if stage == 0 else (stage,)), name
    want = G[f"grid/{name}"]
    same_u16(encode_grid(ctx, G["pos"], want.shape[1]), want, f"{name}: nrf_encode_grid")


@pytest.mark.parametrize("budget", BUDGETS)
def test_encode_grid_bit_exact_under_every_gather_copy_budget(budget):
    desc, keep = model("reference")
    d = nh.ModelDesc.from_buffer_copy(desc)  # (the pointers stay `keep`'s)
    d.gather_copy_budget_mb = budget
    h = nh.NerfHip(0)
    try:
        h.load_model(d)
        want = G["grid/reference"]
        same_u16(encode_grid(h, G["pos"], want.shape[1]), want, f"reference, {budget} MB of gather copies")
    finally:
        h.close()


@pytest.mark.parametrize("name", list(META["dir"]))
def test_encode_dir_against_the_references_kernel(ctx, name):
    desc, keep = model(name)
    assert load(ctx, name, desc)
    want = G[f"dir/{name}"]
    got = encode_dir(ctx, G["dir"], want.shape[1])
    if name.startswith("frequency"):  # __sinf against sinf: the existing bound of test_encode_dir
        np.testing.assert_allclose(got.view(np.float16).astype(np.float32), want.view(np.float16).astype(np.float32), atol=2e-3, rtol=0)
        raw = 6 * int(desc.n_frequencies)
        same_u16(got[:, raw:], want[:, raw:], f"{name}: padding")
    else:
        same_u16(got, want, f"{name}: nrf_encode_dir")


@pytest.mark.parametrize("name", META["net"])
def test_network_and_density_on_the_references_rows(ctx, name):
    desc, keep = model(name)
    assert load(ctx, name, desc)
    xyz, dirs = G["net_xyz"], G["net_dir"]
    feat, dfeat = G[f"net_grid/{name}"], G[f"net_dir/{name}"]
    # the stage entry points expose the features of the very same normalised coordinates: bit for bit
    same_u16(encode_grid(ctx, gen.normalised(xyz), feat.shape[1]), feat, f"{name}: features of the network's positions")
    if not name.endswith("wide"):  # (a Frequency encoding: held at its tolerance above)
        same_u16(encode_dir(ctx, gen.normalised(dirs), dfeat.shape[1]), dfeat, f"{name}: features of the network's directions")
    want = op.Oracle(desc).mlp_forward(feat, dfeat).view(np.float16).astype(np.float32)
    n = len(xyz)
    sg = torch.empty(n, dtype=torch.float32, device="cuda")
    cl = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    x_d, d_d = dev(xyz), dev(dirs)
    torch.cuda.synchronize()
    ctx.network(x_d.data_ptr(), d_d.data_ptr(), n, sg.data_ptr(), cl.data_ptr())
    mlp_close(cl.cpu().numpy(), want[:, :3], f"{name} rgb (network)")
    mlp_close(np.log(sg.cpu().numpy()), np.log(want[:, 3]), f"{name} log sigma (network)")
    sd = torch.empty(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.density(x_d.data_ptr(), n, sd.data_ptr())
    mlp_close(np.log(sd.cpu().numpy()), np.log(want[:, 3]), f"{name} log sigma (density)")
