"""usage (GPU box): python tools/temporal_rate.py [out.txt] -- what temporal accumulation costs on the device
(device.temporal_accumulate, device.denoise_history; wurblpt_amd/csrc/wpt_k_temporal.hip and wpt_k_denoise.hip).

At 1024^2 and 3840x2160, on seeded arrays: one accumulate with a previous history and per-pixel random motion of +-3 pixels (every
lane's taps lie elsewhere: the worst a gather can meet), one with the same offset (0.37, -1.61) in every pixel (what a camera move
or a moving object looks like: neighbouring lanes read neighbouring taps), one accumulate of a first frame (no history to read),
denoise_history with the default parameters, and beside it denoise() of the same frame (which packs first).  Microseconds per
call are the median of CALLS timings between two events (after three untimed calls; enough calls back to back per timing for
about 2^30 pixels), REPEATS times in turn over all operations (A, B, ..., A, B, ...), so that everything alternates; a figure's
spread is (max - min) / median over those repeats.  Beside the accumulate stands the time its compulsory bytes take -- the
current arrays read once (frame, moments, positions, normals 12 bytes each, the map 2, the materials 4, the offsets 8 and 12), one
history read and one written (48 each): 170 bytes per pixel, 122 for a first frame -- at two copy rates.  tools/image_ops_rate.py
measures no rate of its own: it reports its floors with the constant 6.29 TB/s, so the first floor uses that constant, which
makes the ratio comparable with the image operations' recorded ones; the bracketed floor uses the rate of a device-to-device
copy of a buffer of the history's size measured in this call (bytes read plus written over the time).  The plain look-up of the
image operations (resample to the same size, tools/image_ops_rate.py's first line) runs in the same alternation, as the yardstick."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

REPEATS = 3
CALLS = 5
SIZES = ((1024, 1024), (3840, 2160))
BYTES_WITH_HISTORY, BYTES_FIRST_FRAME = 170, 122


def operations(width, height):
    """[(name, callable, compulsory bytes or None)] at one size; the calls go straight to the C ABI with outputs allocated once"""
    import ctypes as C
    import torch
    import image_ops_rate
    from wurblpt_amd import _abi, device
    L = device.lib()
    g = torch.Generator(device="cuda").manual_seed(width)
    rand = lambda *shape: torch.rand(shape, generator=g, device="cuda", dtype=torch.float32)
    px = width * height
    frame = rand(height, width, 3) * 4
    moments = frame * frame * (1.25 + rand(height, width, 3))
    y, x = torch.meshgrid(torch.arange(height, device="cuda", dtype=torch.float32), torch.arange(width, device="cuda", dtype=torch.float32), indexing="ij")
    materials = (((x // 48) * 7 + (y // 32) * 3) % 4).to(torch.int32).contiguous()          # patches of 48 x 32 pixels
    positions = torch.stack([x / 512, y / 512, -2.0 - 0.5 * materials - 0.0005 * x - 0.001 * y], dim=2).contiguous()
    normals = torch.nn.functional.normalize(torch.tensor([0.1, 0.2, 1.0], device="cuda") + (rand(height, width, 3) - 0.5) * 0.1, dim=2).contiguous()
    n_p = torch.full((height, width), 2, dtype=torch.int16, device="cuda").view(torch.uint16)
    offsets = lambda pixel: (pixel, torch.stack([pixel[..., 0] / 512, pixel[..., 1] / 512, -0.0005 * pixel[..., 0] - 0.001 * pixel[..., 1]], dim=2).contiguous())
    pixel, camera = offsets(((rand(height, width, 2) - 0.5) * 6).contiguous())
    pixel_c, camera_c = offsets(torch.tensor([0.37, -1.61], device="cuda").expand(height, width, 2).contiguous())
    guide = (positions, normals, materials)
    previous = device.temporal_accumulate(frame, moments, n_p, guide)
    history, length = device.temporal_accumulate(frame, moments, n_p, guide, (pixel, camera), previous, length_out=True)
    length_c = device.temporal_accumulate(frame, moments, n_p, guide, (pixel_c, camera_c), previous, length_out=True)[1]
    torch.cuda.synchronize()
    kept, kept_c = float((length > 1).float().mean()), float((length_c > 1).float().mean())
    out = torch.empty_like(frame)
    spare = torch.empty_like(history)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    inputs = [ptr(t) for t in (frame, moments, n_p, positions, normals, materials)]
    tp, dp = _abi.TemporalParams(), _abi.DenoiseParams()

    def checked(status):
        assert status == 0, L.wpt_last_error().decode()
    ops = [("accumulate, random motion (%.0f %% of the pixels keep history)" % (100 * kept),
            lambda: checked(L.wpt_postproc_temporal_accumulate(*inputs, ptr(pixel), ptr(camera), ptr(previous), width, height, C.byref(tp), ptr(history), None, stream)),
            px * BYTES_WITH_HISTORY),
           ("accumulate, the same motion everywhere (%.0f %% keep history)" % (100 * kept_c),
            lambda: checked(L.wpt_postproc_temporal_accumulate(*inputs, ptr(pixel_c), ptr(camera_c), ptr(previous), width, height, C.byref(tp), ptr(history), None, stream)),
            px * BYTES_WITH_HISTORY),
           ("accumulate, first frame",
            lambda: checked(L.wpt_postproc_temporal_accumulate(*inputs, None, None, None, width, height, C.byref(tp), ptr(history), None, stream)),
            px * BYTES_FIRST_FRAME),
           ("denoise_history, default parameters (5 iterations)",
            lambda: checked(L.wpt_postproc_denoise_history(ptr(previous), width, height, C.byref(dp), ptr(out), None, stream)), None),
           ("denoise of the same frame, default parameters",
            lambda: checked(L.wpt_postproc_denoise(*inputs, width, height, C.byref(dp), ptr(out), None, stream)), None),
           ("copy of a history's bytes, device to device", lambda: spare.copy_(previous), px * 96)]
    yard, keep = image_ops_rate.operations(width, height)
    ops.append(("image operations' yardstick: " + yard[0][0], yard[0][1], yard[0][2]))
    return ops, [keep, frame, moments, positions, normals, materials, n_p, pixel, camera, pixel_c, camera_c, previous, history, out, spare]


def main():
    import numpy as np
    import torch
    import image_ops_rate
    assert torch.cuda.is_available(), "temporal_rate needs a GPU"
    out = sys.argv[1] if len(sys.argv) > 1 else None
    lines = ["# python tools/temporal_rate.py on %s: microseconds per call (device events; median of %d timings, %d alternating repeats;"
             % (torch.cuda.get_device_name(0), CALLS, REPEATS),
             "# spread = (max - min) / median over the repeats); floor = compulsory bytes over %.2f TB/s (tools/image_ops_rate.py's rate), and"
             % (image_ops_rate.COPY_RATE / 1e12),
             "# the time over that floor; [..] = the same with the copy rate this call measured (image_ops_rate.py measures none: 6.29 TB/s is",
             "# the constant its recorded ratios stand on, the bracketed figures are the floor at the rate of this GPU in this call)"]
    for w, h in SIZES:
        ops, keep = operations(w, h)
        inner = max(1, (1 << 30) // (w * h))
        runs = {name: [] for name, _, _ in ops}
        for _ in range(REPEATS):
            for name, fn, _ in ops:
                runs[name].append(image_ops_rate.timed(fn, inner))
        med = {name: float(np.median(v)) for name, v in runs.items()}
        copy_name = [name for name, _, _ in ops if name.startswith("copy")][0]
        copy_rate = w * h * 96 / (med[copy_name] * 1e-6)
        lines.append("%dx%d (%d calls per timing; measured copy rate %.2f TB/s)" % (w, h, inner, copy_rate / 1e12))
        for name, _, nbytes in ops:
            v = runs[name]
            line = "  %-66s %9.1f us (spread %4.1f %%)" % (name, med[name], 100.0 * (max(v) - min(v)) / med[name])
            if nbytes is not None:
                floor, own = nbytes / image_ops_rate.COPY_RATE * 1e6, nbytes / copy_rate * 1e6
                line += "  floor %7.1f us  x %.2f  [%7.1f us  x %.2f]" % (floor, med[name] / floor, own, med[name] / own)
            lines.append(line)
        del ops, keep
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if out:
        open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
