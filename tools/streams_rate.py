"""usage (GPU box): python tools/streams_rate.py [out.txt] -- a small frame rendered plainly (wpt_render_block_device), split into
K sample streams (wpt_render_split_device) and as a batch of K equal views at the streams' sample count (wpt_render_views_device),
all with the same number of samples per pixel.  A split render is that batch plus one reduce over K * w * h * 12 bytes, so its
time may exceed the batch's by a few per cent at most; its gain over the plain render is what the streams are for.
Every repeat runs all forms of a workload one after another (alternating), REPS repeats after one untimed; medians, and the
repeat spread (max - min) / median of each.  Workloads: the Cornell frame of BASELINE config 2 (GGX + glass, scene in LDS) at
352x288 and the Sponza-class frame (textures, environment map, scene in HBM) at 320x200, both at 16^2 = 256 spp with K = 4, 16,
64; and, for wpt_split_plan's constant, the Cornell frame at 24^2 = 576 spp with every K = k^2 that leaves a stream 2 x 2 strata.
The plan's own choice for the device is marked with *."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from wurblpt_amd import _abi, device, host

REPS = 5


def timed_once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternating(forms, reps=REPS):
    """{name: (median ms, spread)} of `reps` rounds over all forms, one untimed round first"""
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            times[name].append(timed_once(fn))
    return {name: (float(np.median(t)), (max(t) - min(t)) / float(np.median(t))) for name, t in times.items()}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    props = torch.cuda.get_device_properties(0)
    lanes = device.device_lanes()
    lines = ["# tools/streams_rate.py: a frame rendered plainly, split into K sample streams, and as a batch of K equal views (ms, median of %d"
             " alternating repeats; spread = (max - min) / median)" % REPS,
             "# library %s" % bench.library_identity(),
             "# device %s, %d CUs: %d lanes (wpt_device_lanes); wpt_split_plan aims at %d pixels per lane, its choice is marked *"
             % (props.name, props.multi_processor_count, lanes, _abi.SPLIT_PIXELS_PER_LANE),
             "# workload                      n    K  n_s  px/lane  plain ms (spread)  split ms (spread)  batch ms (spread)  split/batch  plain/split"
             "  Msamples/s plain  split"]
    print("\n".join(lines), flush=True)
    stream = torch.cuda.current_stream()
    for label, make, n, ks in (("cornell_352x288", lambda: host.cornell(352, 288, 1, 2), 16, (2, 4, 8)),
                               ("sponza_like_320x200", lambda: host.sponza_like(320, 200), 16, (2, 4, 8)),
                               ("cornell_352x288", lambda: host.cornell(352, 288, 1, 2), 24, (1, 2, 3, 4, 6, 12))):
        sc = make()
        w, h = sc.width, sc.height
        ds = device.DeviceScene(sc)
        cam = _abi.Camera.from_buffer_copy(sc.camera.contents)
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        chosen = device.split_plan(w * h, n, lanes)[0]
        for k in ks:
            K, ns = k * k, n // k
            frames = torch.zeros((K, h, w, 3), dtype=torch.float32, device="cuda")
            cams = [cam] * K
            t = alternating({"plain": lambda: ds.render_block_into(frame, n, stream=stream),
                             "split": lambda: ds.render_split_into(frame, ns, K, stream=stream),
                             "batch": lambda: ds.render_views_into(frames, cams, ns, stream=stream)})
            ds.check()
            samples = w * h * n * n
            lines.append("%-28s  %3d  %3d%s %3d  %7.2f  %9.2f (%4.1f %%)  %9.2f (%4.1f %%)  %9.2f (%4.1f %%)  %11.3f  %11.2f  %16.1f  %5.1f" % (
                label, n, K, "*" if K == chosen else " ", ns, K * w * h / lanes, t["plain"][0], 100 * t["plain"][1], t["split"][0],
                100 * t["split"][1], t["batch"][0], 100 * t["batch"][1], t["split"][0] / t["batch"][0], t["plain"][0] / t["split"][0],
                samples / t["plain"][0] / 1e3, samples / t["split"][0] / 1e3))
            print(lines[-1], flush=True)
            del frames
        ds.close()
        del ds, sc, frame
        torch.cuda.empty_cache()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
