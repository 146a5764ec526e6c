"""The oracle's encodings, index functions and activations, and the library's level table, against the REFERENCE's own code.

oracle/_ref/libref_encodings.so (oracle/ref_encodings.cpp, `make -C oracle ref`) is tiny-cuda-nn's grid.h, spherical_harmonics.h,
frequency.h, identity.h and common_device.h compiled unchanged for the CPU.  Everything here is compared on uint16 / uint32 views
with NO tolerance; without a reference tree (and so without the library) the module is skipped.

What a CPU cannot reproduce: `exp2f` (grid.h:189) and `__sinf` (frequency.h:89) are libm's on both sides, so the comparison is like
for like with the oracle's non-contracted reading and says nothing about the device's intrinsics; positions outside [0, 1] are not
compared ((uint32_t) of a negative floorf is the device's business).

DESIGN.md deviation asserted literally: D-10 (ReLU as a product: NaN and -inf give NaN, a negative value -0).  The comparison
found no disagreement between the oracle and the reference's kernels."""
import importlib.util
import json
import re
from pathlib import Path

import numpy as np
import pytest

import nerfhip as nh
import oracle_py as op
import ref_kernels_py as rk

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module", autouse=True)
def _library():
    rk.require_encodings()


def _generator():
    spec = importlib.util.spec_from_file_location("make_reference_encodings_golden", GOLDEN / "make_reference_encodings_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _generator()
_oracles = {}


def oracle(name):
    if name not in _oracles:
        _oracles[name] = op.Oracle(gen.build(name)[0])
    return _oracles[name]


def same_u16(got, want, what):
    got, want = np.ascontiguousarray(got, np.uint16), np.ascontiguousarray(want, np.uint16)
    assert got.shape == want.shape, f"{what}: shapes {got.shape} != {want.shape}"
    diff = got != want
    if diff.any():
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} fp16 values differ in their bits; first at {at}: "
                             f"oracle {int(got[at]):#06x} reference {int(want[at]):#06x}")


# ------------------------------------------------------------------------------------------------------------ the stand-ins
def test_stand_in_enumerators_are_in_the_references_order():
    """The stand-in headers restate three enums; their values cross the C boundary as integers, so their order is read from the
    reference's headers and compared."""
    if not rk.reference_tree_exists():
        pytest.skip("reads the reference's headers: a library without its tree (built elsewhere) cannot be checked against them")

    def enumerators(path, name):
        text = Path(path).read_text()
        body = re.search(r"enum\s+class\s+" + name + r"\s*\{([^}]*)\}", text).group(1)
        return [e.strip() for e in body.split(",") if e.strip()]

    for header, name in ((rk.TCNN / "common.h", "Activation"), (rk.TCNN / "encoding.h", "InterpolationType"),
                         (rk.TCNN / "encodings" / "grid.h", "GridType")):
        for value, e in enumerate(enumerators(header, name)):
            assert rk.enum_value(f"{name}::{e}") == value, (name, e)


def test_half_addition_through_float_is_the_native_half_addition():
    """oracle/ref_shim/cuda_fp16.h: `+` computes in binary32 and rounds to binary16.  Against the exact sum (binary64 holds it:
    both operands are multiples of 2^-24 below 2^16) rounded once to binary16, over every pair of all 2^16 patterns with 256
    sampled ones -- the sample holds the extremes of every exponent, so that far-apart exponents are met."""
    every = np.arange(1 << 16, dtype=np.uint16)
    rng = np.random.default_rng(3)
    ends = np.array([(e << 10) | m | s for e in range(31) for m in (0, 1, 0x3FF) for s in (0, 0x8000)], np.uint16)  # 186
    some = np.concatenate([ends, rng.integers(0, 1 << 16, 256 - len(ends)).astype(np.uint16)])
    assert len(some) == 256
    for b in some:
        bb = np.full_like(every, b)
        got = rk.half_add(every, bb)
        with np.errstate(over="ignore", invalid="ignore"):
            exact = every.view(np.float16).astype(np.float64) + bb.view(np.float16).astype(np.float64)
            want = exact.astype(np.float16)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got.view(np.float16)), nan)
        assert np.array_equal(got[~nan], want.view(np.uint16)[~nan]), hex(int(b))
    # ... and the oracle's own software conversion agrees with the rounding used as the yardstick above
    vals = rng.normal(size=4096).astype(np.float32) * np.float32(8.0)
    L = op.lib()
    assert [int(L.nrfo_f32_to_f16_soft(float(v))) for v in vals] == [int(x) for x in vals.astype(np.float16).view(np.uint16)]


# ------------------------------------------------------------------------------------------------------------ the grid
def test_the_matrix_holds_the_cases_it_must():
    d = {n: gen.build(n)[0] for n in gen.GRID_MODELS}
    ref = d["reference"]
    if rk.reference_tree_exists():  # the first row IS the reference's configuration (nerf_network.h builds it from this block)
        base = json.loads((rk.REFERENCE / "configs" / "nerf" / "base.json").read_text())["encoding"]
        assert (int(ref.n_levels), int(ref.n_features_per_level), int(ref.log2_hashmap_size), int(ref.base_resolution)) == \
            (base["n_levels"], base["n_features_per_level"], base["log2_hashmap_size"], base["base_resolution"])
        assert "per_level_scale" not in base and "type" not in base and "interpolation" not in base
    assert int(ref.grid_type) == nh.GRID_HASH and int(ref.interpolation) == nh.INTERP["linear"]
    scale = float(ref.per_level_scale)
    assert 1 < scale < 2 and np.log2(scale) != round(np.log2(scale))  # base.json's derived scale: no power of two
    assert {int(m.n_features_per_level) for m in d.values()} == {1, 2, 4, 8}
    assert {int(m.interpolation) for m in d.values()} == {0, 1, 2} and {int(m.grid_type) for m in d.values()} == {0, 1, 2}
    assert any(float(m.per_level_scale) == 2.0 and int(m.grid_type) == 0 for m in d.values())
    assert any((int(m.n_levels) * int(m.n_features_per_level)) % 16 for m in d.values())
    t = nh.level_table(d["tiled-2048"])
    assert int(t.resolution[15]) >= 2048 and int(t.resolution[15]) ** 3 >= 1 << 32
    assert int(d["t12"].log2_hashmap_size) == 12 and int(d["dense-l3"].n_levels) <= 4


@pytest.mark.parametrize("name", list(gen.GRID_MODELS))
def test_encode_grid_is_kernel_grid(name):
    """nrfo_encode_grid against kernel_grid<__half, 3, F> + transpose_encoded_position, launched as GridEncodingTemplated::forward_impl
    launches them, over the offset table the reference's constructor makes and the table of the model's seed"""
    pos = gen.positions()
    assert pos.shape == (264, 3) and pos.min() == 0 and pos.max() == 1
    want, info = gen.reference_grid(name, pos)
    o = oracle(name)
    assert want.shape[1] == o.feat_width
    if name in gen.FIRST_HASHED:  # dense and hashed levels share the model: the level at which hashing starts
        assert info["first_hashed"] == gen.FIRST_HASHED[name], info
    desc = gen.build(name)[0]
    if int(desc.grid_type) != nh.GRID_HASH:
        assert info["first_hashed"] is None
    raw = int(desc.n_levels) * int(desc.n_features_per_level)
    assert (want[:, raw:] == 0).all() and not (want == 0xDEAD).any()  # the padding is written, and written as +0
    same_u16(o.encode_grid(pos), want, f"{name}: grid features")


@pytest.mark.parametrize("name", list(gen.GRID_MODELS))
def test_grid_index_and_fast_hash(name):
    """nrfo_grid_index / nrfo_fast_hash3 against grid_index<3, F> / fast_hash<3>, on corner coordinates up to and including the
    level's resolution, for every level"""
    desc, o = gen.build(name)[0], oracle(name)
    F, L = int(desc.n_features_per_level), int(desc.n_levels)
    offsets, res, _ = rk.grid_table(F, L, int(desc.log2_hashmap_size), int(desc.base_resolution), float(desc.per_level_scale), int(desc.grid_type))
    rng = np.random.default_rng(4)
    for level in range(L):
        r = int(res[level])
        axis = sorted({0, 1, 2, r // 2, r - 1, r} | {int(v) for v in rng.integers(0, r + 1, 3)})
        corners = np.array([[x, y, z] for x in axis for y in axis for z in axis], np.uint32)
        want = rk.grid_index(F, int(desc.grid_type), int(offsets[level + 1] - offsets[level]), r, corners)
        got = np.array([o.grid_index(level, int(x), int(y), int(z)) for x, y, z in corners], np.uint32)
        assert np.array_equal(got * np.uint32(F), want), (name, level)
    corners = rng.integers(0, 1 << 32, (4096, 3), dtype=np.uint64).astype(np.uint32)
    corners[:8] = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2048, 2048, 2048], [0xFFFFFFFF] * 3, [1, 1, 1], [2047, 0, 2048]]
    L_ = op.lib()
    got = np.array([L_.nrfo_fast_hash3(int(x), int(y), int(z)) for x, y, z in corners], np.uint32)
    assert np.array_equal(got, rk.fast_hash3(corners))


# ------------------------------------------------------------------------------------------------------------ the level table
def _desc(F, L, log2T, base, scale, grid_type):
    d = nh.ModelDesc()
    d.abi_version = nh.NRF_ABI_VERSION
    d.grid_type, d.n_levels, d.n_features_per_level, d.log2_hashmap_size = grid_type, L, F, log2T
    d.base_resolution, d.per_level_scale = base, scale
    return d


@pytest.mark.parametrize("grid_type", [nh.GRID_HASH, nh.GRID_DENSE, nh.GRID_TILED])
def test_level_table_is_the_constructors(grid_type):
    """nrf_level_table_compute (host code, no GPU) against the GridEncodingTemplated constructor (grid.h:875-940): every offset and
    every resolution, and a refusal exactly where the constructor throws.  log2 T 4..24, base resolutions 2..64, 1..16 levels,
    F in {1, 2, 4, 8}; per-level scales 2 (exp2f exact), base.json's derived one and 1.5."""
    scales = [2.0, float(gen.build("reference")[0].per_level_scale), 1.5]
    n = 0
    for log2T in range(4, 25) if grid_type == nh.GRID_HASH else (4, 19):  # (the constructor reads log2 T for Hash only)
        for base in (2, 3, 5, 8, 16, 17, 33, 64):
            for scale in scales:
                for F in (1, 2, 4, 8):
                    for L in range(1, 17):
                        ref = rk.grid_table(F, L, log2T, base, scale, grid_type)
                        d = _desc(F, L, log2T, base, np.float32(scale), grid_type)
                        try:
                            t = nh.level_table(d)
                        except nh.NerfHipError:
                            t = None
                        what = (grid_type, log2T, base, scale, F, L)
                        assert (t is None) == (ref is None), f"{what}: one of the two refuses this model"
                        if ref is None:
                            continue
                        offsets, res, n_params = ref
                        assert list(t.offset[:L + 1]) == [int(v) for v in offsets], what
                        assert list(t.resolution[:L]) == [int(v) for v in res], what
                        assert n_params == (int(offsets[L]) * F) % (1 << 32)  # (the constructor keeps it in 32 bits)
                        n += 1
    assert n > 3000


# ------------------------------------------------------------------------------------------------------------ directions
@pytest.mark.parametrize("name", list(gen.DIR_MODELS))
def test_encode_dir_is_the_references_kernel(name):
    """nrfo_encode_dir against kernel_sh (degree 1..8), frequency_encoding (1..6 frequencies) and identity, padding columns included"""
    d01 = gen.directions()
    assert d01.shape == (4096, 3) and d01.min() >= 0 and d01.max() <= 1
    o = oracle(name)
    want = gen.reference_dir(name, d01)
    assert want.shape[1] == o.dir_width and not (want == 0xDEAD).any()
    same_u16(o.encode_dir(d01), want, f"{name}: direction features")


# ------------------------------------------------------------------------------------------------------------ activations
@pytest.mark.parametrize("act", sorted(rk.ACTIVATIONS))
def test_activation_is_warp_activation(act):
    """nrfo_activation (on the fp16 value, rounded to fp16 as the oracle's MLP stores it) against warp_activation<__half> over all
    65 536 inputs.  NaN results are compared as NaN (a payload is no number); everything else bit for bit."""
    bits = np.arange(1 << 16, dtype=np.uint16)
    want = rk.activation(act, bits)
    L = op.lib()
    vals = bits.view(np.float16).astype(np.float32)
    with np.errstate(over="ignore"):  # (exp of a large value: +inf in fp16, as in the reference)
        got = np.array([L.nrfo_activation(act, float(v)) for v in vals], np.float32).astype(np.float16).view(np.uint16)
    nan_w, nan_g = np.isnan(want.view(np.float16)), np.isnan(got.view(np.float16))
    assert np.array_equal(nan_w, nan_g), f"activation {act}: NaN at different inputs"
    assert np.array_equal(got[~nan_w], want[~nan_w]), f"activation {act}"
    if act == nh.ACT["relu"]:
        # D-10, literally: the reference's ReLU is x * (half)(x > 0) -- NaN stays NaN, -inf becomes NaN, a negative value -0
        # (the HIP path clamps with max(x, 0) and gives +0 for all three: tests/test_parity_gpu.py pins that side)
        x = bits.view(np.float16)
        assert nan_w[np.isnan(x)].all() and nan_w[bits == 0xFC00].all() and nan_w.sum() == np.isnan(x).sum() + 1
        neg = (bits > 0x8000) & (bits < 0xFC00)
        assert (want[neg] == 0x8000).all() and want[0x8000] == 0x8000 and want[0] == 0
        pos = (bits > 0) & (bits <= 0x7C00)
        assert np.array_equal(want[pos], bits[pos])


# ------------------------------------------------------------------------------------------------------------ the fixture
def test_golden_vectors_regenerate_to_the_committed_bytes(tmp_path):
    """tests/golden/reference_encodings.npz, regenerated from the library: the same members in the same order, every member's .npy
    bytes equal (compared uncompressed)"""
    committed = GOLDEN / "reference_encodings.npz"
    assert committed.stat().st_size <= 1 << 19
    out = tmp_path / "reference_encodings.npz"
    gen.write(out)
    fresh, kept = gen.read_members(out), gen.read_members(committed)
    assert [n for n, _ in fresh] == [n for n, _ in kept]
    stale = [n for (n, a), (_, b) in zip(fresh, kept) if a != b]
    assert not stale, f"tests/golden/reference_encodings.npz is stale in {stale}: run tests/golden/make_reference_encodings_golden.py"
