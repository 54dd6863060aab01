"""Pixels in slices (wpt_set_slices, FEAT_SLICED kernels): a pooled launch of the kernels with the scene in LDS cuts every pixel
into units of strata rows and hands out all first units, then all second units, ...; a unit goes on where the one before it
stopped, whichever lane runs it.  The frame is the frame of the launch with one lane per pixel (variant bit 0x10) bit for bit,
for every number of units, mapping of lanes to pixels and form of the kernel, and whichever of the two lanes that meet at a
unit's start runs it; every unit behind a pixel's first is run exactly once (wpt_last_slice_stats)."""
import numpy as np
import pytest

from wurblpt_amd import host

pytestmark = pytest.mark.gpu

W, H = 1024, 640          # 655 360 pixels against 262 144 lanes in flight on an MI355X: the smallest frame the pool hands out


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


@pytest.fixture(scope="module")
def scene():
    return host.cornell(W, H, 1, 2)


@pytest.fixture(scope="module")
def ds(dev, scene):
    return dev.DeviceScene(scene)


@pytest.fixture(scope="module")
def references(dev, ds):
    """frames of the launch with one lane per pixel (no pool, so nothing is sliced), by (samples_sqrt, randomize); made once"""
    cache = {}

    def get(s, randomize=1):
        if (s, randomize) not in cache:
            dev.lib().wpt_set_launch_config(0, 0x10)
            try:
                p = host.default_params()
                p.randomize_ray_over_pixel = randomize
                frame, _ = ds.render(s, params=p)
                assert dev.lib().wpt_last_render_passes() == 1 and dev.last_slice_stats() == (0, 0)
                assert b"sliced" not in dev.lib().wpt_kernel_form()
            finally:
                dev.lib().wpt_set_launch_config(0, 0)
            frame.setflags(write=False)
            cache[(s, randomize)] = frame
        return cache[(s, randomize)]
    return get


def bits_differing(a, b):
    assert a.shape == b.shape
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def units_of(s, n):
    rows = -(-s // n)
    return -(-s // rows)


def render_sliced(dev, ds, s, n, flags=0, params=None, walk=0):
    """(frame, units the launch reports, taken, continued) of a launch under wpt_set_slices(n | flags)"""
    try:
        dev.set_slices(n | flags)
        dev.lib().wpt_set_walk(walk)
        frame, _ = ds.render(s, params=params)          # synchronises and checks the scene
        form = dev.lib().wpt_kernel_form().decode()
        assert dev.lib().wpt_last_render_passes() == 1
        taken, continued = dev.last_slice_stats()
    finally:
        dev.set_slices(0)
        dev.lib().wpt_set_walk(0)
    ds.check()
    units = int(form.split("sliced x")[1]) if "sliced x" in form else 1
    return frame, units, taken, continued, form


@pytest.mark.parametrize("n", [0, 2, 4, 8])
def test_eight_rows_in_any_number_of_units(dev, ds, references, n):
    got, units, taken, continued, form = render_sliced(dev, ds, 8, n)
    import torch
    lanes_at_once = torch.cuda.get_device_properties(0).multi_processor_count * 1024
    plan_units, plan_rows = dev.slices_plan(W * H, lanes_at_once, 8)
    assert units == (plan_units if n == 0 else units_of(8, n)) and units >= 2, (form, plan_units, plan_rows)
    assert form.startswith("rotated corners, sliced x")
    print("s=8 n=%d: units %d taken %d continued %d" % (n, units, taken, continued))
    assert bits_differing(got, references(8)) == 0
    assert taken + continued == W * H * (units - 1)


def test_default_launch_renders_the_oracles_rows(dev, ds, scene, oracle):
    rows = (311, 8)                                        # eight rows across the boxes
    block = (rows[0] * W, rows[1] * W)
    ref, _ = oracle.render(scene, 8, block=block)
    got, units, _, _, _ = render_sliced(dev, ds, 8, 0)
    assert units >= 2
    assert ref[rows[0]:rows[0] + rows[1]].any()
    assert bits_differing(got[rows[0]:rows[0] + rows[1]], ref[rows[0]:rows[0] + rows[1]]) == 0


def test_units_of_unequal_length(dev, ds, references):
    """seven rows in units of 3, 3 and 1"""
    got, units, taken, continued, _ = render_sliced(dev, ds, 7, 3)
    assert units == 3
    assert bits_differing(got, references(7)) == 0
    assert taken + continued == W * H * 2


def test_the_lane_that_finds_its_next_unit_declined_runs_it(dev, ds, references):
    """WPT_SLICES_DECLINE_ODD: no unit of a pixel on an odd slot is taken over, so the lane that rendered the pixel's first unit
    runs all the others straight on"""
    got, units, taken, continued, _ = render_sliced(dev, ds, 8, 4, flags=dev.SLICES_DECLINE_ODD)
    assert units == 4
    print("decline odd: taken %d continued %d" % (taken, continued))
    assert bits_differing(got, references(8)) == 0
    assert taken + continued == W * H * (units - 1)
    assert continued >= (W * H // 2) * (units - 1)


def test_ragged_blocks_and_bands(dev, ds, references):
    """the cuts and the two band shapes of test_pixel_pool_never_changes_results: tiled, untiled and ragged mappings"""
    import torch
    ref = references(8)
    frame = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    try:
        dev.set_slices(4)
        cuts = [0, 8 * W * 40, 8 * W * 40 + 300001, W * H]   # tiled, untiled (ragged), untiled
        forms = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            ds.render_block_into(frame, 8, (a, b - a))
            forms.append(dev.lib().wpt_kernel_form())
            t, c = dev.last_slice_stats()
            if b"sliced" in forms[-1]:
                assert t + c == (b - a) * 3, (a, b, t, c)
            assert dev.lib().wpt_last_render_passes() == 1
        torch.cuda.synchronize()
        ds.check()
        assert any(b"sliced x4" in f for f in forms), forms      # the blocks that are larger than the device are sliced
        assert bits_differing(frame.cpu().numpy(), ref) == 0
        for band_rows, stride in ((8, 2), (5, 2)):            # tiled and untiled bands
            total = np.zeros_like(ref)
            for rank in range(stride):
                frame.zero_()
                ds.render_bands_into(frame, 8, band_rows, rank, stride, stream=torch.cuda.current_stream())
                torch.cuda.synchronize()
                assert b"sliced x4" in dev.lib().wpt_kernel_form() and dev.lib().wpt_last_render_passes() == 1
                mine = sum(min(band_rows, H - b * band_rows) for b in range(rank, -(-H // band_rows), stride)) * W
                t, c = dev.last_slice_stats()
                assert t + c == mine * 3, (band_rows, rank, t, c, mine)
                total += frame.cpu().numpy()
            ds.check()
            assert bits_differing(total, ref) == 0, band_rows
    finally:
        dev.set_slices(0)


def test_the_select_form(dev, ds, references):
    got, units, taken, continued, form = render_sliced(dev, ds, 8, 4, walk=dev.WALK_SELECT_CORNERS)
    assert form == ", sliced x4"
    assert bits_differing(got, references(8)) == 0
    assert taken + continued == W * H * 3


def test_pixel_centres(dev, ds, references):
    """randomize_ray_over_pixel = 0: the camera ray draws nothing, so the generator's state at a unit's end is another"""
    p = host.default_params()
    p.randomize_ray_over_pixel = 0
    got, units, taken, continued, _ = render_sliced(dev, ds, 8, 4, params=p)
    assert units == 4
    assert bits_differing(got, references(8, 0)) == 0
    assert taken + continued == W * H * 3


def test_variant_0x40_never_slices(dev, ds, references):
    dev.lib().wpt_set_launch_config(0, 0x40)
    try:
        got, units, taken, continued, form = render_sliced(dev, ds, 8, 4)
    finally:
        dev.lib().wpt_set_launch_config(0, 0)
    assert form == "rotated corners" and (taken, continued) == (0, 0)
    assert bits_differing(got, references(8)) == 0


def test_a_render_that_is_not_sliced_reports_no_slice_statistics(dev, ds, references):
    """wpt_last_slice_stats is the most recent render call's: behind a sliced launch, a forced wavefront render and a stage of a
    session both report (0, 0), and render their block of the unpooled frame bit for bit"""
    import torch
    rows = slice(311, 315)                                 # a block of 64 x 64 pixels: four rows across the boxes
    block = (rows.start * W, 64 * 64)
    ref = references(2)
    assert ref[rows].any()
    _, units, taken, continued, _ = render_sliced(dev, ds, 8, 4)
    assert units == 4 and taken + continued == W * H * 3
    dev.lib().wpt_set_wavefront(1, 0, 0, 0)
    try:
        wf, _ = ds.render(2, block=block)
        name, stats = dev.lib().wpt_kernel_name(), dev.last_slice_stats()
    finally:
        dev.lib().wpt_set_wavefront(0, 0, 0, 0)
    assert stats == (0, 0) and name == b"wf_trace + wf_shade"
    assert bits_differing(wf[rows], ref[rows]) == 0
    _, units, taken, continued, _ = render_sliced(dev, ds, 8, 4)
    assert units == 4 and taken + continued == W * H * 3
    frame = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    session = ds.progressive(2, block=block)
    try:
        assert session.advance(2, frame) == 2
        torch.cuda.synchronize()
        ds.check()
        assert dev.last_slice_stats() == (0, 0) and dev.lib().wpt_last_render_passes() == 1
        assert dev.lib().wpt_kernel_name() == b"wpt_pathtrace" and dev.lib().wpt_kernel_form() == b"rotated corners"
    finally:
        session.close()
    assert bits_differing(frame.cpu().numpy()[rows], ref[rows]) == 0
