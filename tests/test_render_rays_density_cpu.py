"""NRF_RAYS_DENSITY_ONLY, the parts that need no GPU: the constant in the header and in the Python binding, the flag's definition
stated on the checker (tests/rays_clip_oracle.py run with a network whose colour is zero), and the built library's device code:
every RAYS instance that renders float planes has a density-only twin with fewer MFMAs and fewer code bytes."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import nerfhip as nh
import rays_clip_oracle as rco
import rays_forms as rf
import test_render_rays_clip_cpu as ccpu

ROOT = Path(__file__).resolve().parent.parent


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_constant_is_4_in_the_header_and_in_the_binding():
    header = (ROOT / "include" / "nerfhip.h").read_text()
    m = re.search(r"\bNRF_RAYS_DENSITY_ONLY\s*=\s*(\w+)", header)
    assert m is not None and int(m.group(1), 0) == 4 == nh.NRF_RAYS_DENSITY_ONLY
    assert int(re.search(r"\bNRF_RAYS_DEPTH_T\s*=\s*(\w+)", header).group(1), 0) == 1 == nh.NRF_RAYS_DEPTH_T
    assert nh.NRF_ABI_VERSION == 7  # an addition: no new exported symbol, no new structure member


class _SigmaOnly:
    """The oracle with a colour network that returns zero: what a density-only instance evaluates."""

    def __init__(self, oracle):
        self._oracle = oracle
        self.coloured = 0

    def march(self, *a, **kw):
        return self._oracle.march(*a, **kw)

    def composite(self, *a, **kw):
        return self._oracle.composite(*a, **kw)

    def network(self, *a, **kw):
        sigma, rgb = self._oracle.network(*a, **kw)
        self.coloured += int(np.count_nonzero(np.any(np.asarray(rgb) != 0, axis=-1)))
        return sigma, np.zeros_like(rgb)


def _scenes(name):
    if name == "bound1":
        desc, keep, orc, o, d, full = ccpu._scene("bound1")
    else:
        desc, keep, orc, o, d, full = rf.scene(name)
    return desc, orc, o, d, full


@pytest.mark.parametrize("scene", ["bound1", "sine-h30"])
def test_the_definition_on_the_checker(scene):
    """A statement about the reference semantics (it holds with or without the feature): with the colour of every sample zero, the
    per-ray loop yields the same weight sums and depths, bit for bit, and rgb = (1 - weight_sum) * background."""
    desc, orc, o, d, full = _scenes(scene)
    n = len(o)
    W, H = rf.RW, rf.RH
    assert n == W * H
    t = rco.ramp(W, H)
    yy, xx = np.divmod(np.arange(n), W)
    bg = np.stack([xx / W, 0.1 + 0.8 * yy / H, 0.25 + 0.125 * ((3 * xx + 5 * yy) % 7)], axis=1).astype(np.float32)
    rgba, depth, ns, raw = rco.render(orc, desc, o, d, t_max=t, background=bg)
    proxy = _SigmaOnly(orc)
    rgba_d, depth_d, ns_d, raw_d = rco.render(proxy, desc, o, d, t_max=t, background=bg)
    assert ns == ns_d > 1000 and proxy.coloured > 0.5 * ns  # (the colours that were dropped were not zero anyway)
    assert np.array_equal(_bits(rgba_d[:, 3]), _bits(rgba[:, 3]))
    assert np.array_equal(_bits(depth_d), _bits(depth)) and np.array_equal(_bits(raw_d), _bits(raw))
    T = (np.float32(1) - rgba_d[:, 3]).astype(np.float32)
    assert np.array_equal(rgba_d[:, :3], (T[:, None] * bg).astype(np.float32))
    # what the flag removes is visible in the scene: on the unlimited frame (the scalar bg_color of the default options) the colour
    # network moves at least 40 % of the pixels it touches by more than 0.05 -- the condition the GPU tests assert of their scenes
    a_full = full[0][:, 3]
    hit = a_full > 0
    through = ((np.float32(1) - a_full).astype(np.float32) * np.float32(nh.default_options().bg_color)).astype(np.float32)
    share = float(np.mean(np.any(np.abs(full[0][hit, :3] - through[hit, None]) > 0.05, axis=1)))
    print(f"{scene}: samples {ns} under the ramp, colour network visible on {share:.3f} of the unlimited frame's hit pixels")
    assert share >= 0.4


def _device_symbols(tmp_path):
    """demangled kernel name -> (v_mfma_f32_16x16x32_f16 instructions, code bytes) of the gfx950 code objects inside libnerfhip.so"""
    llvm = Path("/opt/rocm/lib/llvm/bin")
    if not (llvm / "clang-offload-bundler").exists() or shutil.which("objcopy") is None:
        pytest.skip("ROCm LLVM tools not available")
    lib = ROOT / "nerf-cuda_amd" / "libnerfhip.so"
    fat = tmp_path / "fat.bin"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(lib), str(fat)], check=True)
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
    mfma, size = {}, {}
    for i, a in enumerate(starts):
        part, co = tmp_path / f"fat{i}.bin", tmp_path / f"dev{i}.co"
        part.write_bytes(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.run([str(llvm / "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={part}", f"--output={co}"], check=True)
        if not co.stat().st_size:
            continue
        cur = None
        for ln in subprocess.run([str(llvm / "llvm-objdump"), "-d", str(co)], check=True, capture_output=True, text=True).stdout.splitlines():
            m = re.match(r"^[0-9a-f]+ <([^>]+)>:", ln)
            if m:
                cur = m.group(1)
                mfma[cur] = 0
            elif cur is not None and ln.startswith("\t") and ln.split() and ln.split()[0].startswith("v_mfma_f32_16x16x32_f16"):
                mfma[cur] += 1
        # the symbol table: address, flags (F: a function), section, size, [visibility,] name
        for ln in subprocess.run([str(llvm / "llvm-objdump"), "-t", str(co)], check=True, capture_output=True, text=True).stdout.splitlines():
            f = ln.split()
            if ".text" in f and "F" in f[1:f.index(".text")]:
                size[f[-1]] = int(f[f.index(".text") + 1], 16)
    syms = [s for s in mfma if s in size]
    names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.splitlines()
    return {n.split("(")[0]: (mfma[s], size[s]) for s, n in zip(syms, names)}


def test_every_float_rays_instance_has_a_lighter_density_only_twin(tmp_path):
    syms = _device_symbols(tmp_path)
    pairs = []
    for name, fig in syms.items():
        m = re.search(r"\b(render_kernel|render_persistent_kernel)<([^>]*)>", name)
        if not m:
            continue
        args = [a.strip() for a in m.group(2).split(",")]
        at = 4 if m.group(1) == "render_kernel" else 5  # the RAYS argument: 0 pinhole, 1 rays, 2 density-only rays
        if args[at] != "2":
            continue
        assert args[-1] == "false" or m.group(1) == "render_kernel"  # (FAST stays last, and off)
        twin = name.replace(m.group(0), f"{m.group(1)}<{', '.join(args[:at] + ['1'] + args[at + 1:])}>")
        assert twin in syms, (name, twin)
        pairs.append((name, fig, syms[twin]))
    persistent = [p for p in pairs if "render_persistent_kernel" in p[0]]
    assert len(pairs) == 13 and len(persistent) == 3, [p[0] for p in pairs]
    for name, (mf, nb), (mf_full, nb_full) in pairs:
        print(f"{name}: MFMA {mf} of {mf_full}, code bytes {nb} of {nb_full}")
        assert 0 < mf < mf_full, (name, mf, mf_full)
        assert 0 < nb < nb_full, (name, nb, nb_full)
    # every float-plane RAYS instance is some pair's full twin: 3 persistent ones (the 8-bit ones have none) and 10 per-strip ones
    full = [n for n in syms if (m := re.search(r"\b(render_kernel|render_persistent_kernel)<([^>]*)>", n))
            and [a.strip() for a in m.group(2).split(",")][4 if m.group(1) == "render_kernel" else 5] == "1"]
    assert len(full) == 16, full
