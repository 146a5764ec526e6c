"""The rows of tests/rays_forms.py, the parts that need no GPU: every row reaches the march form and the table placement it names
(nrf_debug_march_form), the ramp scene of tests/test_render_rays_forms_gpu.py cuts every row's frame partly, fully and not at
all on the checker -- the conditions that keep the GPU tests from passing vacuously -- and the checker and the assembled oracle
are pinned on generic geometries as tests/test_render_rays_clip_cpu.py and tests/test_render_rays_cpu.py pin them at H = 32."""
import numpy as np
import pytest

import nerfhip as nh
import oracle_py as op
import rays_clip_oracle as rco
import rays_forms as rf
import rays_oracle as ro
import synthetic as syn

W, H = rf.RW, rf.RH


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("row", list(rf.ROWS))
def test_every_row_reaches_the_march_form_it_names(row):
    kw, stage, want, _ = rf.ROWS[row]
    desc, keep, _ = rf.build(row)
    assert (desc.density_grid_size, desc.cascade, desc.bound) == (kw["H"], kw.get("cascade", 1), np.float32(kw.get("bound", 1.0)))
    assert rf.march_form(desc.density_grid_size, desc.cascade, desc.bound) == want, row
    # the coarse level is the grid side's alone; the persistent form needs it
    assert want[1] == (1 if kw["H"] % 4 == 0 else 0)
    assert rf.schedules(row) == (["persistent", "strip"] if stage == rf.HOT and want[1] else ["strip"])


def test_the_rows_cover_the_instances_the_small_models_do_not():
    """Read against launch_persistent_rays and launch_strip_rays (nrf_kernels_rays.hip): (stage, form, tables in LDS) of the rows."""
    got = {(v[1],) + v[2] for v in rf.ROWS.values()}
    assert got == {(rf.HOT, rf.GENERIC, 1), (rf.HOT, rf.GENERIC, 0), (rf.WIDE, rf.POW2, 1), (rf.WIDE, rf.GENERIC, 1),
                   (rf.WIDE, rf.GENERIC, 0), (rf.GEN, rf.GENERIC, 1), (rf.GEN, rf.GENERIC, 0)}
    # the models of tests/test_render_rays_gpu.py and tests/test_render_rays_clip_gpu.py are the other two forms
    assert rf.march_form(32, 1, 1.0) == (rf.UNIT, 1) and rf.march_form(32, 3, 4.0) == (rf.POW2, 1)
    # every fast-forward function of the GENERIC form: one cascade at bound 1, several cascades, one cascade below bound 1
    shapes = {(rf.kwargs(r).get("cascade", 1) > 1, rf.kwargs(r).get("bound", 1.0) < 1.0) for r in rf.FF_ROWS}
    assert shapes == {(False, False), (True, False), (False, True)}
    assert all(rf.ROWS[r][2] == (rf.GENERIC, 1) for r in rf.FF_ROWS) and all(rf.ROWS[r][2] == (rf.GENERIC, 0) for r in rf.NO_COARSE_ROWS)


@pytest.mark.parametrize("row", list(rf.ROWS))
def test_the_ramp_cuts_every_row_partly_fully_and_not_at_all(row):
    """A condition on the GPU tests' inputs, checked on the oracle alone: as t_max the ramp t(px) = 0.7 + 0.9 px / W leaves pixels
    partly cut, fully cut and untouched; as t_min it leaves pixels partly cut.  The figures are the table's (to its three digits)."""
    (hit, partly, fully, untouched, partly_min), (fn, n, n2) = rf.ramp_figures(row)
    print(f"{row}: hit {hit:.3f} t_max partly {partly:.3f} fully {fully:.3f} untouched hit pixels {untouched:.3f} samples {n} of {fn}; "
          f"t_min partly {partly_min:.3f} samples {n2}")
    assert partly >= 0.04 and partly_min >= 0.04
    assert untouched >= 0.04
    assert fully >= (0.07 if row in rf.SINE_ROWS else 0.2)
    assert 0 < n < fn and 0 < n2 < fn
    assert np.allclose((hit, partly, fully, untouched, partly_min), rf.ROWS[row][3], rtol=0, atol=0.00051), row


@pytest.mark.parametrize("row", list(rf.ROWS))
def test_a_limit_misplaced_by_one_march_step_is_far_beyond_the_tolerance(row):
    """What the GPU tests' 2 / 255 can see, on the checker alone: the ramp moved by the march's smallest step, 2 sqrt(3) / max_steps
    -- a clamp, a cascade interval or a fast-forward start that is one sample off -- moves some pixel of every row's frame by
    more than ten times the tolerance (measured: 48 / 255 on sine-h96, 115 / 255 .. 251 / 255 on the other rows)."""
    desc, keep, orc, o, d, full = rf.scene(row)
    step = np.float32(2.0 * np.sqrt(3.0) / nh.default_options().max_steps)
    for kind in ("t_max", "t_min"):
        t, (want, wdepth, n, raw) = rf.checked(row, kind)[4:6]
        rgba = rco.render(orc, desc, o, d, **{kind: (t + step).astype(np.float32)})[0]
        moved = float(np.abs(rgba - want).max())
        print(f"{row} {kind}: one step moves the frame by {moved * 255:.1f} / 255")
        assert moved >= 20.0 / 255.0, (row, kind)


@pytest.mark.parametrize("row", ["h64-b1.5-c2", "h30-b4-c3"])
def test_checker_without_limits_is_the_rays_oracle_bit_for_bit(row):
    desc, keep, orc, o, d, (want, wdepth, wn) = rf.scene(row)
    rgba, depth, ns, raw = rco.render(orc, desc, o, d)
    assert ns == wn and ns > 1000
    assert np.array_equal(_bits(rgba), _bits(want)) and np.array_equal(_bits(depth), _bits(wdepth))


def test_assembled_oracle_reproduces_the_per_ray_render_on_a_generic_geometry():
    """tests/test_render_rays_cpu.py's pin of the assembled oracle, at three cascades of a grid side and a bound that are no powers of two."""
    desc, keep, orc, o, d, (rgba, depth, n) = rf.scene("h48-b3-c3")
    cam, pose = syn.default_camera(W, H), syn.orbit_pose(30, 30)
    opts = nh.default_options()
    want, wdepth, wst = orc.render(cam, pose, W, H, opts, schedule=op.SCHED_PER_RAY)
    o2, d2, nr, fr = orc.generate_rays(cam, pose, W, H, opts)
    assert np.array_equal(_bits(o2), _bits(o)) and np.array_equal(_bits(d2), _bits(d))
    near, far = ro.near_far([desc.aabb[i] for i in range(6)], o, d, opts.min_near)
    assert np.array_equal(_bits(near), _bits(nr)) and np.array_equal(_bits(far), _bits(fr))
    assert n == wst.n_samples and n > 1000, (n, wst.n_samples)
    assert np.array_equal(_bits(rgba.reshape(H, W, 4)), _bits(want)) and np.array_equal(_bits(depth.reshape(H, W)), _bits(wdepth))
