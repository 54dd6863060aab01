"""usage (GPU box): python tools/image_ops_rate.py [out.txt] -- what the image operations of the output side cost on the device
(device.resample, lens_warp, despeckle, distance_to_coords; wurblpt_amd/csrc/wpt_k_image_ops.hip).

Each operation at 1024^2 and 3840x2160 on seeded images: microseconds per call are the median of CALLS timings between two events
(after three untimed calls; enough calls back to back per timing for about 2^30 pixels), REPEATS times in turn over all operations
(A, B, ..., A, B, ...), so that the two forms of despeckle and everything else alternate; a figure's spread is (max - min) / median
over those repeats.  Beside each time stands its floor: the bytes the operation must read plus the bytes it must write, computed
from the shapes, over 6.29 TB/s, the copy rate measured on this GPU (a bilinear look-up counts its source image once: the four
taps of neighbouring pixels are the same texels).  Despeckle's two forms are selected with wpt_set_despeckle_form; the line at the
end says which is faster, and WPT_DESPECKLE_TILE in wpt_k_image_ops.hip is set from it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 3
CALLS = 5
SIZES = ((1024, 1024), (3840, 2160))
COPY_RATE = 6.29e12  # bytes per second
FRUSTUM = (-0.625, 0.75, -0.1875, 0.15625)
LENSES = (("none", (0, 0, 0, 0, 0, 0)), ("radial_and_planar", (1, 0.5, 0.125, 0.0, 0.03125, -0.015625)),
          ("radial_only", (2, 0.375, 0.0625, 0.015625, 0.0, 0.0)), ("opencv", (3, 0.25, 0.0625, 0.0078125, 0.015625, -0.0078125)))


# notes on the run recorded in profiles/image_ops_rate.txt (a build with the gather form as its default): which form each operation
# takes and what stands between it and the floor; what has not been profiled is marked as supposed
NOTES = [
    "# forms: every operation is one launch with one lane per output pixel in workgroups of 32 x 8, no scratch.",
    "#   resample, lens warp, distance to coordinates: the four taps of the look-up are plain loads, one dword per component, so a",
    "#     3-component pixel is twelve dword loads and three dword stores at a 12-byte stride between lanes; that strided access and, at",
    "#     1024^2, the launch itself (a plain look-up lasts 4.5 to 10 us) are supposed to be what keeps the plain look-up at 1.7 x the floor at",
    "#     3840x2160 (not profiled).  A quarter of the output pixels takes 0.4 of the time (x 1.08 of its own floor): the lanes, not the source's bytes, set it.",
    "#   lens models: the closed forms add 10 to 25 us at 3840x2160; distort costs more than the closed-form inverses, supposedly",
    "#     because its coordinates spread further over the source.  The OpenCV inverse is the out-of-line iteration (wptlens::undistortCall): it",
    "#     doubles the call (110.6 against 53.2 us), and a wave runs as long as its slowest lane.",
    "#   despeckle: nine taps of three dwords per pixel and 81 comparisons for the ranks; the tile form (the workgroup's pixels and",
    "#     their ring through 4 KB of LDS) against the gather form is the pair of figures above: equal at 1024^2, the tile form",
    "#     2.5 us (3.6 %) faster at 3840x2160 at spreads of 0.3 and 0.5 %, so WPT_DESPECKLE_TILE is 1.",
    "#   distance to coordinates: one source component, three written; a square root and three divisions per pixel, correctly rounded.",
]


def operations(width, height):
    """[(name, callable, bytes read + written)] at one size; the calls go straight to the C ABI with outputs allocated once, so that
    a timing holds as little host work as a caller can get away with"""
    import ctypes as C
    import torch
    from wurblpt_amd import device, host
    L = device.lib()
    g = torch.Generator(device="cuda").manual_seed(width)
    rgb = torch.rand((height, width, 3), generator=g, device="cuda", dtype=torch.float32)
    rgb[torch.rand((height, width), generator=g, device="cuda") < 0.02] *= 50.0
    dist = 1.0 + 4.0 * torch.rand((height, width, 1), generator=g, device="cuda", dtype=torch.float32)
    out = torch.empty_like(rgb)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p_rgb, p_dist, p_out = (C.c_void_p(t.data_ptr()) for t in (rgb, dist, out))
    keep = [rgb, dist, out]
    px = width * height

    def checked(status):
        assert status == 0, L.wpt_last_error().decode()
    ops = [("resample to the same size, 3 components", lambda: checked(L.wpt_postproc_resample(p_rgb, width, height, 3, width, height, p_out, stream)), px * 24),
           ("resample to half the size, 3 components",
            lambda: checked(L.wpt_postproc_resample(p_rgb, width, height, 3, width // 2, height // 2, p_out, stream)), px * 12 + px // 4 * 12)]
    for name, k in LENSES:
        cam = host.lens_camera(FRUSTUM, *k)
        keep.append(cam)
        for forward in (1, 0):
            ops.append(("lens warp %s %s, 3 components" % (name, "forward (undistort)" if forward else "back (distort)"),
                        lambda cam=cam, forward=forward: checked(L.wpt_postproc_lens_warp(p_rgb, width, height, 3, C.byref(cam), forward, p_out, stream)),
                        px * 24))
    for form in (0, 1):
        def run(form=form):
            L.wpt_set_despeckle_form(form)
            checked(L.wpt_postproc_despeckle(p_rgb, width, height, 3, 1.25, p_out, stream))
        ops.append(("despeckle %s" % ("gather", "tile")[form], run, px * 24))
    for name, k in (LENSES[0], LENSES[3]):
        cam = host.lens_camera(FRUSTUM, *k)
        keep.append(cam)
        ops.append(("distance to coordinates %s, 1 component" % name,
                    lambda cam=cam: checked(L.wpt_postproc_distance_to_coords(p_dist, width, height, 1, C.byref(cam), 1, p_out, stream)), px * 16))
    return ops, keep


def timed(fn, inner):
    import numpy as np
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1000.0 / inner)
    return float(np.median(times))


def main():
    import numpy as np
    import torch
    from wurblpt_amd import device
    assert torch.cuda.is_available(), "image_ops_rate needs a GPU"
    out = sys.argv[1] if len(sys.argv) > 1 else None
    lines = ["# python tools/image_ops_rate.py on %s: microseconds per call (device events; median of %d timings, %d alternating repeats;"
             % (torch.cuda.get_device_name(0), CALLS, REPEATS),
             "# spread = (max - min) / median over the repeats), the floor (bytes read + written over 6.29 TB/s) and the time over the floor"]
    verdict = []
    for w, h in SIZES:
        ops, keep = operations(w, h)
        inner = max(1, (1 << 30) // (w * h))
        runs = {name: [] for name, _, _ in ops}
        for _ in range(REPEATS):
            for name, fn, _ in ops:
                runs[name].append(timed(fn, inner))
        device.set_despeckle_form(-1)
        lines.append("%dx%d (%d calls per timing)" % (w, h, inner))
        med = {}
        for name, _, nbytes in ops:
            v = runs[name]
            med[name] = float(np.median(v))
            floor = nbytes / COPY_RATE * 1e6
            lines.append("  %-58s %9.1f us (spread %4.1f %%)  floor %7.1f us  x %.2f" % (name, med[name], 100.0 * (max(v) - min(v)) / med[name], floor, med[name] / floor))
        verdict.append("%dx%d gather %.1f us, tile %.1f us" % (w, h, med["despeckle gather"], med["despeckle tile"]))
    lines.append("# despeckle: " + "; ".join(verdict) + "; the library was built with the %s form" % device.despeckle_form())
    lines += NOTES
    text = "\n".join(lines) + "\n"
    if out:
        open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
