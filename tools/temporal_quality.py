"""usage (GPU box): python tools/temporal_quality.py [out.txt] -- what temporal accumulation (device.temporal_accumulate,
device.denoise_history) does to the error of a sequence's frames.  Recorded, not asserted (profiles/temporal_quality.txt): no
test holds a bound on these figures, and the parameters are the defaults, untuned.

Every frame is a split render of 4 streams x 2^2 samples (16 spp) with its stream moment film, so samples_sqrt = 2 for the
denoiser; the relative L2 error sqrt(sum (f - ref)^2 / sum ref^2) against a 2304-spp render is given for the last frame alone, for
that frame filtered (device.denoise: the path without accumulation), for the accumulated frame and for the accumulated frame
filtered (device.denoise_history), all with the default parameters.
  Cornell 64 x 64, at rest (NULL motion), 8 frames: frame f from the streams 4 f .. 4 f + 3 (a frame seed), and again with the streams
  0 .. 3 in every frame, which is what accumulation does without frame seeds: eight copies of one estimate.
  host.animated 64 x 64 with a static camera and moving instances, 8 frames 1 / 30 apart up to t = 0.5, guide and both offset arrays
  from ground_truth_device(times = (t, t - 1 / 30, t)), frame seeds: the same four figures over the pixels whose history survived all
  eight frames (N = 8) and over the pixels that were reset on the way (N < 8), each against the reference's norm over the same pixels.
  In that scene the lamp slides as well, so the light on every surface changes from frame to frame, which the rule does not detect
  (max_history is the only guard); the last line is the same room with nothing moving (variant 6), through the same calls."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 8
SIZE = 64
DT = 1.0 / 30


def rel(f, ref, mask=None):
    import numpy as np
    f, ref = f.cpu().numpy().astype(np.float64), ref.astype(np.float64)
    if mask is not None:
        f, ref = f[mask], ref[mask]
    return float(np.sqrt(((f - ref) ** 2).sum() / (ref ** 2).sum()))


def render(ds, first, params=None):
    import torch
    frame = torch.zeros((SIZE, SIZE, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros_like(frame)
    ds.render_split_into(frame, 2, 4, first=first, moments=moments, params=params)
    return frame, moments


def cornell(seeded):
    import numpy as np
    import torch
    from wurblpt_amd import _abi, device, host
    ds = device.DeviceScene(host.cornell(SIZE, SIZE))
    guide = ds.first_hit_colours_device()
    history = None
    for f in range(FRAMES):
        frame, moments = render(ds, 4 * f if seeded else 0)
        history, length = device.temporal_accumulate(frame, moments, 2, guide, None, history, length_out=True)
    ref = np.asarray(ds.render(48)[0]).reshape(SIZE, SIZE, 3)
    torch.cuda.synchronize()
    ds.check()
    figures = (rel(frame, ref), rel(device.denoise(frame, moments, 2, guide), ref),
               rel(device.denoise_history(history, _abi.DenoiseParams(iterations=0)), ref), rel(device.denoise_history(history), ref))
    assert float(length.min()) == FRAMES
    ds.close()
    return figures


def animated(variant=2):
    import numpy as np
    import torch
    from wurblpt_amd import _abi, device, host
    bits = sum(1 << device.GT_NAMES.index(n) for n in device.GUIDE_NAMES + device.MOTION_NAMES)
    history = None
    for f in range(FRAMES):
        t = 0.5 - (FRAMES - 1 - f) * DT
        ds = device.DeviceScene(host.animated(SIZE, SIZE, variant, t, t))
        p = host.default_params()
        p.t0 = p.t1 = t
        truth = ds.ground_truth_device(bits=bits, params=p, times=(t, t - DT, t))
        frame, moments = render(ds, 4 * f, p)
        history, length = device.temporal_accumulate(frame, moments, 2, truth, truth if f else None, history, length_out=True)
        torch.cuda.synchronize()
        ds.check()
        if f < FRAMES - 1:
            ds.close()
    ref = np.asarray(ds.render(48, params=p)[0]).reshape(SIZE, SIZE, 3)
    N = length.cpu().numpy()
    kept = N == FRAMES
    fields = (frame, device.denoise(frame, moments, 2, truth), device.denoise_history(history, _abi.DenoiseParams(iterations=0)),
              device.denoise_history(history))
    torch.cuda.synchronize()
    ds.close()
    return [tuple(rel(f, ref, mask) for f in fields) for mask in (None, kept, ~kept)], int(kept.sum()), int((~kept).sum()), float(N[~kept].mean()) if (~kept).any() else 0.0


def main():
    import torch
    assert torch.cuda.is_available(), "temporal_quality needs a GPU"
    out = sys.argv[1] if len(sys.argv) > 1 else None
    row = lambda name, v: "%s : %.5f : %.5f : %.5f : %.5f : %.4f : %.4f" % (name, v[0], v[1], v[2], v[3], v[2] / v[0], v[3] / v[1])
    lines = ["# python tools/temporal_quality.py on %s: %d frames of 16 spp (4 streams x 2^2) at %d x %d against 2304 spp, default parameters;"
             % (torch.cuda.get_device_name(0), FRAMES, SIZE, SIZE), "# relative L2 error sqrt(sum (f - ref)^2 / sum ref^2)",
             "# case : last frame : last frame filtered (denoise) : accumulated : accumulated filtered (denoise_history) : accumulated over frame : accumulated filtered over frame filtered"]
    lines.append(row("cornell at rest, streams 4 f .. 4 f + 3 in frame f", cornell(True)))
    lines.append(row("cornell at rest, streams 0 .. 3 in every frame", cornell(False)))
    rows, kept, lost, mean_lost = animated()
    lines.append(row("animated (static camera, moving instances), all pixels", rows[0]))
    lines.append(row("animated, the %d pixels whose history survived all frames (N = %d)" % (kept, FRAMES), rows[1]))
    lines.append(row("animated, the %d pixels reset on the way (N < %d, mean N %.2f)" % (lost, FRAMES, mean_lost), rows[2]))
    rows, kept, lost, _ = animated(6)
    lines.append(row("the animated room with everything at rest (variant 6: the lamp does not slide), offsets from the same pass: %d pixels with N = %d, %d reset"
                     % (kept, FRAMES, lost), rows[0]))
    text = "\n".join(lines) + "\n"
    if out:
        open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
