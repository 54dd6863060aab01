"""usage (GPU box): python tools/transient_rate.py [out.txt] -- cost of the transient film (SensorRGBTransient,
wpt_render_transient_block_device): Msamples/s of the plain render against one transient render with K = 16 / 64 / 256 path
length bins, and against K gated renders (the reference's way: one SensorRGB render per bin).  The K gated renders are not run:
4 gated renders are timed and their time is scaled by K / 4 (every gated render is a plain render with other gate values).
Workloads: the Cornell frame of BASELINE config 2 (1024^2, GGX + glass, 64 spp) and the Sponza-class frame (1920x1080, 16 spp)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from wurblpt_amd import device, host

REPS = 3


def timed(fn, reps=REPS):
    """median milliseconds of `reps` runs of fn() on the current stream, after one untimed run"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    lines = ["# tools/transient_rate.py: the transient film against the plain render and against K gated renders (median of %d)" % REPS,
             "# library %s" % bench.library_identity(),
             "# 'K gated' = the measured time of 4 gated renders (SensorRGB path-length gates, the plain kernel) x K / 4",
             "# workload                       K    plain ms  transient ms  x plain  K gated ms  gated/transient  Msamples/s (transient)  kernel"]
    print("\n".join(lines), flush=True)
    for label, make, S, span in (("cornell_1024_64spp", lambda: host.cornell(1024, 1024, 1, 2), 8, 16.0),
                                 ("sponza_like_1920x1080_16spp", lambda: host.sponza_like(1920, 1080), 4, 64.0)):
        sc = make()
        w, h = sc.width, sc.height
        ds = device.DeviceScene(sc)
        stream = torch.cuda.current_stream()
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        plain_ms = timed(lambda: ds.render_block_into(frame, S, stream=stream))
        plain_kernel = device.lib().wpt_kernel_name().decode()
        gates = []
        for k in range(4):
            p = host.default_params()
            p.min_path_len = float(np.float32(span * k / 4))
            p.max_path_len = float(np.nextafter(np.float32(span * (k + 1) / 4), np.float32(-np.inf)))
            gates.append(p)
        gated4_ms = timed(lambda: [ds.render_block_into(frame, S, params=p, stream=stream) for p in gates])
        samples = w * h * S * S
        lines.append("%-28s  %4s  %9.2f  %12s  %7s  %10s  %15s  %22.1f  %s" % (label, "-", plain_ms, "-", "-", "-", "-", samples / plain_ms / 1e3, plain_kernel))
        print(lines[-1], flush=True)
        for K in (16, 64, 256):
            edges = device.uniform_edges(0.0, span / K, K)
            bins = torch.zeros((K, h, w, 3), dtype=torch.float32, device="cuda")
            t_ms = timed(lambda: ds.render_transient_into(frame, bins, S, edges, stream=stream))
            ds.check()
            gated_ms = gated4_ms * K / 4
            lines.append("%-28s  %4d  %9.2f  %12.2f  %7.2f  %10.1f  %15.1f  %22.1f  %s" % (
                label, K, plain_ms, t_ms, t_ms / plain_ms, gated_ms, gated_ms / t_ms, samples / t_ms / 1e3, device.lib().wpt_kernel_name().decode()))
            print(lines[-1], flush=True)
            del bins
            torch.cuda.empty_cache()
        ds.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
