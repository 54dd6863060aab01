"""usage (GPU box): python tools/shutter_rate.py [out.txt] [--plain] -- what the rolling shutter costs.  host.animated variant 0
(camera, cube, panel and lamp move) at 1024 x 768 and 8^2 samples per pixel, bounded for [0, 1], rendered three ways over that
one span: the plain render over [0, 1]; a rolling frame read from the top with rows exposed for 0.25 (t0 = 0, t1 = 0.25,
row_time = 0.75 / 767); a rolling frame of instant rows (t0 = t1 = 0, row_time = 1 / 767).  All three run the moving-scene
kernel; the rule adds a few vector instructions per camera ray, so the rates should agree within the spread of the repeats.
The three alternate, REPS times after one untimed round; per way the median, the fastest and the slowest run.
--plain: the plain render alone, which a library without the shutter has too (WPT_LIB_DIR selects a second build of the
libraries, e.g. the parent's): one line, for an A/B of the moving-scene kernel between two builds from alternating processes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from wurblpt_amd import device, host

W, H, S, REPS = 1024, 768, 8, 7


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
    plain_only = "--plain" in sys.argv
    props = torch.cuda.get_device_properties(0)
    scene = host.animated(W, H, 0, 0.0, 1.0)
    ds = device.DeviceScene(scene)
    frame = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()

    def params(t0, t1):
        p = host.default_params()
        p.t0, p.t1 = t0, t1
        return p
    over_span = params(0.0, 1.0)
    ways = [("plain render over [0, 1]", lambda: ds.render_block_into(frame, S, None, over_span, None, stream))]
    if not plain_only:
        blurred, rows = host.shutter(0.75 / (H - 1), True), params(0.0, 0.25)
        instant, instants = host.shutter(1.0 / (H - 1), True), params(0.0, 0.0)
        for sh, p in ((blurred, rows), (instant, instants)):
            first, last = device.shutter_span(sh, p.t0, p.t1, H)
            assert first == 0.0 and abs(float(last) - 1.0) < 1e-5, (first, last)
        ways.append(("rolling, rows exposed for 0.25, read over 0.75", lambda: ds.render_shutter_into(frame, S, blurred, None, rows, None, stream)))
        ways.append(("rolling, instant rows, read over 1", lambda: ds.render_shutter_into(frame, S, instant, None, instants, None, stream)))
    kernels = []
    for _, render in ways:  # untimed: code objects, first touches
        render()
        torch.cuda.synchronize()
        kernels.append(device.lib().wpt_kernel_name().decode())
    times = [[] for _ in ways]
    for _ in range(REPS):
        for k, (_, render) in enumerate(ways):
            times[k].append(timed_once(render))
    ds.check()
    lines = ["# tools/shutter_rate.py: host.animated variant 0, %d x %d, %d spp, bounded for [0, 1]; %d alternating runs per way after one untimed" % (W, H, S * S, REPS),
             "# library %s" % bench.library_identity(),
             "# device %s, %d CUs" % (props.name, props.multi_processor_count),
             "# way                                              median ms   fastest   slowest  Msamples/s (median)  kernel"]
    for (label, _), t, kernel in zip(ways, times, kernels):
        ms = float(np.median(t))
        lines.append("%-50s %9.2f %9.2f %9.2f  %10.1f           %s" % (label, ms, min(t), max(t), W * H * S * S / ms / 1e3, kernel))
    if not plain_only:
        base = float(np.median(times[0]))
        spread = (max(times[0]) - min(times[0])) / base
        lines.append("# spread of the plain render's runs: %.2f %% of its median; rolling / plain (medians): %s" % (
            100.0 * spread, ", ".join("%.4f" % (float(np.median(t)) / base) for t in times[1:])))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
