"""usage (GPU box): python tools/tof_rate.py [out.txt] -- cost of the time-of-flight sensor (wpt_render_tof_block_device).
Two questions, each answered by alternating repeats in one process:
  1. one phase image against the twin scene's SensorRGB render in the same kernel family (the twin has a LightSpot where the ToF
     scene has its LightTof, so both trace the same paths): the accumulate rule is the whole difference;
  2. four phase images in one launch against four one-phase launches (the reference's way).
Workloads: the wall-and-box scene (tof_scene variant 2, Cornell class) at 1024^2 x 256 spp, the room of wurblpt-tof-example
(variant 0) at the reference sensor's 352x288 and at 1920x1080, 100 spp.  The RGB twin of variant 2 has a two-sided spot light
and so runs in the all-features kernel; the ToF launch is timed there too (kernel word 0x02) and in its own kernel with the
scene in LDS."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from wurblpt_amd import device, host

REPS = 5


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternating(fns, reps=REPS):
    """milliseconds of every function of `fns`, run in turn `reps` times after one untimed round: {name: [ms, ...]}"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(once(fn))
    return times


def med(x):
    return float(np.median(x))


def spread(x):
    return (max(x) - min(x)) / med(x)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    lines = ["# tools/tof_rate.py: the time-of-flight sensor against its RGB twin, and four phases in one launch against four launches",
             "# (alternating repeats in one process, median of %d; spread = (max - min) / median)" % REPS,
             "# library %s" % bench.library_identity()]
    print("\n".join(lines), flush=True)
    stream = torch.cuda.current_stream()
    sensor = host.tof_sensor()
    for label, variant, w, h, S, words in (("wall_and_box_1024x1024_256spp", 2, 1024, 1024, 16, (0x02, 0)),
                                           ("tof_room_352x288_100spp", 0, 352, 288, 10, (0,)),
                                           ("tof_room_1920x1080_100spp", 0, 1920, 1080, 10, (0,))):
        tof, twin = device.DeviceScene(host.tof_scene(w, h, variant, 0)), device.DeviceScene(host.tof_scene(w, h, variant, 1))
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        plane = torch.zeros((1, h, w, 3), dtype=torch.float32, device="cuda")
        planes = torch.zeros((4, h, w, 3), dtype=torch.float32, device="cuda")
        samples = w * h * S * S
        for word in words:
            device.lib().wpt_set_launch_config(0, word)
            try:
                fns = {"rgb_twin": lambda: twin.render_block_into(frame, S, stream=stream),
                       "tof_1": lambda: tof.render_tof_into(plane, S, sensor, phases=[0], stream=stream),
                       "tof_4": lambda: tof.render_tof_into(planes, S, sensor, stream=stream),
                       "tof_4x1": lambda: [tof.render_tof_into(plane, S, sensor, phases=[j], stream=stream) for j in range(4)]}
                fns["rgb_twin"]()
                rgb_kernel = device.lib().wpt_kernel_name().decode()
                fns["tof_1"]()
                tof_kernel = device.lib().wpt_kernel_name().decode()
                t = alternating(fns)
            finally:
                device.lib().wpt_set_launch_config(0, 0)
            tof.check()
            lines.append("%s, kernel word %#x: RGB twin on '%s', ToF on '%s'" % (label, word, rgb_kernel, tof_kernel))
            for name in fns:
                lines.append("    %-9s %9.2f ms  spread %5.1f %%  %8.1f Msamples/s" % (name, med(t[name]), 100 * spread(t[name]), samples / med(t[name]) / 1e3))
            lines.append("    one phase / RGB twin = %.3f   (spreads %.1f %% and %.1f %%)" % (
                med(t["tof_1"]) / med(t["rgb_twin"]), 100 * spread(t["tof_1"]), 100 * spread(t["rgb_twin"])))
            lines.append("    four phases in one launch / four launches = %.3f   (a quarter would be 0.250); / one phase = %.3f" % (
                med(t["tof_4"]) / med(t["tof_4x1"]), med(t["tof_4"]) / med(t["tof_1"])))
            print("\n".join(lines[-7:]), flush=True)
        tof.close()
        twin.close()
        del frame, plane, planes
        torch.cuda.empty_cache()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
