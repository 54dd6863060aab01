"""usage (GPU box): python tools/views_rate.py [out.txt] -- a batch of views (wpt_render_views_device) against the same views
rendered one after another by plain renders (wpt_render_block_device, one launch per view, all on one stream).  Msamples/s,
median of 5 runs after one untimed run.  Workloads:
  - the Cornell frame of BASELINE config 2 (GGX + glass, scene in LDS) at 352x288 and 100 spp: V views on a turntable, +-40
    degrees around the point the scene's camera looks at;
  - the Sponza-class frame (textures, environment map, scene in HBM) at 320x200 and 64 spp: V views panned +-40 degrees about
    the scene's camera position (a turntable would leave the building);
  - for scale, the plain render of one full-size frame of each (1024^2 and 1920x1080, same sample counts).
V = 1 is the cost of the per-lane camera: the same launch as the plain render but for the camera's words, which the batch
reads from device memory and the plain render from the kernel arguments."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from wurblpt_amd import device, host

REPS = 5
VIEWS = (1, 4, 16, 64)


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


def rotate(q, v):
    u, w = np.array(q[0:3], np.float64), float(q[3])
    v = np.array(v, np.float64)
    return v + 2.0 * w * np.cross(u, v) + 2.0 * np.cross(u, np.cross(u, v))


def yaw(v, a):
    return np.array([v[0] * np.cos(a) + v[2] * np.sin(a), v[1], -v[0] * np.sin(a) + v[2] * np.cos(a)])


def cameras(sc, n, orbit):
    """orbit: n eyes on an arc of +-40 degrees around the looked-at point; otherwise n directions panned about the eye"""
    base = sc.camera.contents
    eye = np.array(base.translation, np.float64)
    fwd = rotate(base.rotation, (0.0, 0.0, -1.0))
    dist = max(1.0, float(np.linalg.norm(eye)))
    centre = eye + dist * fwd
    cams = []
    for i in range(n):
        a = np.radians(-40.0 + 80.0 * i / (n - 1)) if n > 1 else 0.0
        if orbit:
            cams.append(host.camera_looking_at(sc, centre + yaw(eye - centre, a), centre, (0.0, 1.0, 0.0)))
        else:
            cams.append(host.camera_looking_at(sc, eye, eye + dist * yaw(fwd, a), (0.0, 1.0, 0.0)))
    return cams


def plain_views(ds, frames, cams, S, stream):
    """the V views as plain renders, one launch each, in order on one stream"""
    cam = ds.host.camera
    saved = type(cam.contents).from_buffer_copy(cam.contents)
    try:
        for v, c in enumerate(cams):
            cam[0] = c
            ds.render_block_into(frames[v], S, stream=stream)
    finally:
        cam[0] = saved


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    lanes = device.lib()
    props = torch.cuda.get_device_properties(0)
    lanes_at_once = props.multi_processor_count * 4 * 4 * 64
    lines = ["# tools/views_rate.py: a batch of V views in one launch against V plain renders on one stream (Msamples/s, median of %d)" % REPS,
             "# library %s" % bench.library_identity(),
             "# device %s, %d CUs: %d lanes in flight at 4 waves per SIMD" % (props.name, props.multi_processor_count, lanes_at_once),
             "# workload                        V  px/lane  plain x V ms  batch ms  Msamples/s plain  Msamples/s batch  speed-up  kernel (batch)"]
    print("\n".join(lines), flush=True)
    stream = torch.cuda.current_stream()
    for label, make, full, S, orbit in (
            ("cornell_352x288_100spp", lambda: host.cornell(352, 288, 1, 2), lambda: host.cornell(1024, 1024, 1, 2), 10, True),
            ("sponza_like_320x200_64spp", lambda: host.sponza_like(320, 200), lambda: host.sponza_like(1920, 1080), 8, False)):
        sc = make()
        w, h = sc.width, sc.height
        ds = device.DeviceScene(sc)
        for V in VIEWS:
            cams = cameras(sc, V, orbit)
            frames = torch.zeros((V, h, w, 3), dtype=torch.float32, device="cuda")
            plain_ms = timed(lambda: plain_views(ds, frames, cams, S, stream))
            batch_ms = timed(lambda: ds.render_views_into(frames, cams, S, stream=stream))
            ds.check()
            kernel = lanes.wpt_kernel_name().decode()
            samples = V * w * h * S * S
            lines.append("%-30s  %3d  %7.2f  %12.2f  %8.2f  %16.1f  %16.1f  %8.2f  %s" % (
                label, V, V * w * h / lanes_at_once, plain_ms, batch_ms, samples / plain_ms / 1e3, samples / batch_ms / 1e3,
                plain_ms / batch_ms, kernel))
            print(lines[-1], flush=True)
            del frames
        ds.close()
        del ds, sc
        torch.cuda.empty_cache()
        big = full()
        dsb = device.DeviceScene(big)
        frame = torch.zeros((big.height, big.width, 3), dtype=torch.float32, device="cuda")
        full_ms = timed(lambda: dsb.render_block_into(frame, S, stream=stream))
        samples = big.width * big.height * S * S
        lines.append("%-30s  %3s  %7.2f  %12.2f  %8s  %16.1f  %16s  %8s  %s" % (
            "  full frame %dx%d" % (big.width, big.height), "-", big.width * big.height / lanes_at_once, full_ms, "-",
            samples / full_ms / 1e3, "-", "-", lanes.wpt_kernel_name().decode()))
        print(lines[-1], flush=True)
        dsb.close()
        del dsb, big, frame
        torch.cuda.empty_cache()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
