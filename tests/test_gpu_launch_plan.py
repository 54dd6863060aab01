"""wpt_launch_plan against what ran: the plan for the facts of a launch and the device's own compute-unit count says what
wpt_last_render_passes, wpt_kernel_form and wpt_kernel_name report behind the render.  The shapes are the smallest that cross
`lanes` and `2 * lanes` on a device of 256 compute units, where the plan must be the named strategy; on a device with fewer
units the plan, not a constant, says what to expect."""
import numpy as np
import pytest

from wurblpt_amd import host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def compute_units():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


GGX, GLASS, ALL = 32, 64, 2303  # feature bits (wpt_device.h)


def planned(dev, scene, need, sensor, pixels, samples_sqrt):
    """the plan for the launch's facts as the library has them: whether its kernel keeps the scene in LDS is wpt_kernel_choice's
    answer for the scene's own counts, and that kernel must be the one that ran"""
    d = scene.d
    name, form, _, lds_bytes, _ = dev.kernel_choice(need, sensor, False, d.node_count, d.tri_count, d.material_count)
    assert dev.lib().wpt_kernel_name().decode() == name and dev.lib().wpt_kernel_form().decode().startswith(form)
    return dev.launch_plan(sensor, False, need, lds_bytes > 0, pixels, samples_sqrt, compute_units()), lds_bytes > 0


def ran_as_planned(dev, plan, pixels, strategy_at_256):
    name, form = dev.lib().wpt_kernel_name().decode(), dev.lib().wpt_kernel_form().decode()
    passes, stats = dev.lib().wpt_last_render_passes(), dev.last_slice_stats()
    print(plan, name, form, passes, stats)
    if compute_units() == 256:
        assert plan["strategy"] == strategy_at_256 and plan["pooled"]
    assert not plan["wavefront"] and name.startswith("wpt_pathtrace")
    assert passes == plan["passes"] == (2 if plan["strategy"] == "two passes" else 1)
    if plan["strategy"] == "sliced":
        assert form.endswith(", sliced x%d" % plan["units"]) and stats[0] + stats[1] == pixels * (plan["units"] - 1)
    else:
        assert "sliced" not in form and stats == (0, 0)
    return name, form


def test_cornell_box_in_slices(dev):
    w, h, s = 1024, 512, 8
    sc = host.cornell(w, h, 1, 2)
    frame, _ = dev.DeviceScene(sc).render(s)
    plan, in_lds = planned(dev, sc, GGX | GLASS, dev.SENSOR_FRAME, w * h, s)
    _, form = ran_as_planned(dev, plan, w * h, "sliced")
    assert in_lds and form.startswith("rotated corners") and np.isfinite(frame).all() and frame.any()      # the kernel with the scene in LDS


def test_sponza_like_in_two_passes(dev):
    w, h, s = 1536, 1024, 8
    sc = host.sponza_like(w, h, seed=3, detail=0.03, tex_size=16, env_width=32, importance_n=8)
    frame, _ = dev.DeviceScene(sc).render(s)
    plan, in_lds = planned(dev, sc, ALL, dev.SENSOR_FRAME, w * h, s)
    name, form = ran_as_planned(dev, plan, w * h, "two passes")
    assert not in_lds and (name, form) == ("wpt_pathtrace", "") and np.isfinite(frame).all() and frame.any()   # a kernel that fetches the scene from HBM


def test_adaptive_map_in_its_order(dev):
    w, h = 512, 256
    sc = host.cornell(w, h, 1, 2)
    counts = (1 + (np.arange(w * h).reshape(h, w) // 7) % 2).astype(np.uint16)                   # ones and twos
    frame = dev.DeviceScene(sc).render_adaptive(counts).cpu().numpy()
    plan, in_lds = planned(dev, sc, GGX | GLASS, dev.SENSOR_ADAPTIVE, w * h, 1)
    name, _ = ran_as_planned(dev, plan, w * h, "adaptive order")
    assert in_lds and "adaptive, scene in LDS" in name and np.isfinite(frame).all() and frame.any()
