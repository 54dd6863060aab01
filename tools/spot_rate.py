"""usage (GPU box): python tools/spot_rate.py [out.txt] -- cost of LightSpot: Msamples/s of each spot scene (host.spot_scene)
against its diffuse twin (every LIGHT_SPOT record retyped LIGHT_DIFFUSE) rendered by the same kernel, the all-features one
(launch variant 0x02 for the twin), and against the twin in the kernel the library picks for it (also the all-features
one: the Cornell twins keep the light's MaterialTwoSided).  Frames of 1024^2 at 64 spp."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from wurblpt_amd import _abi, device, host

REPS = 5
S = 8


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


def rate(sc, variant=0):
    """(Msamples/s, kernel name) of one frame of `sc` under launch variant `variant`"""
    w, h = sc.width, sc.height
    device.lib().wpt_set_launch_config(0, variant)
    try:
        ds = device.DeviceScene(sc)
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream()
        ms = timed(lambda: ds.render_block_into(frame, S, stream=stream))
        ds.check()
        kernel = device.lib().wpt_kernel_name().decode()
        ds.close()
    finally:
        device.lib().wpt_set_launch_config(0, 0)
    return w * h * S * S / ms / 1e3, kernel


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    lines = ["# tools/spot_rate.py: spot scenes against their diffuse twins, 1024^2 x %d spp (median of %d)" % (S * S, REPS),
             "# library %s" % bench.library_identity(),
             "# scene                        spot Msamples/s  twin, same kernel  spot/twin  twin, own kernel  kernels (spot | twin own)"]
    print("\n".join(lines), flush=True)
    for label, variant in (("cornell_white_spot", 0), ("stage", 1), ("cornell_ggx_glass_spot", 2)):
        sc = host.spot_scene(1024, 1024, variant)
        spot, spot_kernel = rate(sc)
        for i in range(sc.d.material_count):
            if sc.d.materials[i].type == _abi.MAT_LIGHT_SPOT:
                sc.d.materials[i].type = _abi.MAT_LIGHT_DIFFUSE
        twin_full, twin_full_kernel = rate(sc, 0x02)
        assert twin_full_kernel == spot_kernel, (twin_full_kernel, spot_kernel)
        twin_own, twin_own_kernel = rate(sc)
        lines.append("%-28s  %15.1f  %17.1f  %9.3f  %16.1f  %s | %s" % (label, spot, twin_full, spot / twin_full, twin_own, spot_kernel, twin_own_kernel))
        print(lines[-1], flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
