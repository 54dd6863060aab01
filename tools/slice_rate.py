"""usage (GPU box): python tools/slice_rate.py [out.txt] [--sweep] -- the end of a launch of the kernel with the scene in LDS, and
what handing pixels out in slices (wpt_set_slices) does to it.  Msamples/s of the Cornell frame of BASELINE config 2 (GGX +
glass) at one total of samples in three shapes: 1024^2 x 1024 spp (4 pixels per lane on an MI355X), 2048^2 x 256 spp (16) and
4096^2 x 64 spp (64); median of 5 runs after one untimed run.  The more pixels per lane, the smaller the part of the launch in
which lanes run out of work one by one: the difference between the rows is the cost of that end.  With a library that has
wpt_set_slices every shape is measured with the library's plan and unsliced; --sweep adds the bench frame at 1, 2, 4, 8 and 15
units per pixel, alternating, three runs each, with the units taken over and run on with (wpt_last_slice_stats) beside each.
WPT_LIB_DIR selects a second build of the libraries (wurblpt_amd/device.py), e.g. the parent's."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from wurblpt_amd import device, host

REPS = 5
SHAPES = ((1024, 32), (2048, 16), (4096, 8))
SWEEP = (1, 2, 4, 8, 15)


def timed_once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else None
    L = device.lib()
    can_slice = hasattr(L, "wpt_set_slices")
    props = torch.cuda.get_device_properties(0)
    lanes_at_once = props.multi_processor_count * 4 * 4 * 64
    lines = ["# tools/slice_rate.py: the Cornell frame (GGX + glass, scene in LDS) at one total of samples in three shapes (Msamples/s, median of %d)" % REPS,
             "# library %s" % bench.library_identity(),
             "# device %s, %d CUs: %d lanes in flight at 4 waves per SIMD" % (props.name, props.multi_processor_count, lanes_at_once),
             "# frame        spp  px/lane  slices        ms  Msamples/s  all runs (ms)                          kernel form"]
    print("\n".join(lines), flush=True)
    stream = torch.cuda.current_stream()
    for side, S in SHAPES:
        sc = host.cornell(side, side, 1, 2)
        ds = device.DeviceScene(sc)
        frame = torch.zeros((side, side, 3), dtype=torch.float32, device="cuda")
        for setting in ((0, 1) if can_slice else (None,)):
            if setting is not None:
                device.set_slices(setting)
            render = lambda: ds.render_block_into(frame, S, stream=stream)
            render()
            torch.cuda.synchronize()
            times = [timed_once(render) for _ in range(REPS)]
            ds.check()
            ms = float(np.median(times))
            lines.append("%4dx%-6d %5d  %7.2f  %-8s %8.2f  %10.1f  %-38s %s" % (
                side, side, S * S, side * side / lanes_at_once, {None: "-", 0: "plan", 1: "never"}[setting], ms, side * side * S * S / ms / 1e3,
                " ".join("%.2f" % t for t in times), L.wpt_kernel_form().decode()))
            print(lines[-1], flush=True)
        if can_slice:
            device.set_slices(0)
        ds.close()
        del ds, sc, frame
        torch.cuda.empty_cache()
    if can_slice and "--sweep" in sys.argv:
        side, S = SHAPES[0]
        sc = host.cornell(side, side, 1, 2)
        ds = device.DeviceScene(sc)
        frame = torch.zeros((side, side, 3), dtype=torch.float32, device="cuda")
        render = lambda: ds.render_block_into(frame, S, stream=stream)
        lines.append("# sweep: %dx%d x %d spp under wpt_set_slices(n), alternating, one untimed run first" % (side, side, S * S))
        lines.append("# round   n  units        ms  Msamples/s      taken  continued")
        print("\n".join(lines[-2:]), flush=True)
        render()
        torch.cuda.synchronize()
        for rnd in range(3):
            for n in SWEEP:
                device.set_slices(n)
                ms = timed_once(render)
                form = L.wpt_kernel_form().decode()
                taken, continued = device.last_slice_stats()
                lines.append("%7d  %2d  %5s  %8.2f  %10.1f  %9d  %9d" % (
                    rnd, n, form.split("sliced x")[1] if "sliced x" in form else "1", ms, side * side * S * S / ms / 1e3, taken, continued))
                print(lines[-1], flush=True)
        device.set_slices(0)
        ds.check()
        ds.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
