"""What tests/test_shutter.py and tests/test_gpu_shutter.py share: the rolling shutter's rule restated in numpy float32 (one
rounding per operation, as include/wurblpt_hip.h states it), the frame every GPU case renders, and parameter records."""
import numpy as np

from wurblpt_amd import device, host

F32 = np.float32
W, H, S = 32, 24, 3  # several groups of 8 rows, every row with an interval of its own; a per-row reference takes milliseconds


def rule(t0, t1, row_time, from_top, height, y):
    """(a, b) of frame row y (0 = bottom): k = from_top ? height - 1 - y : y; s = (float)k * row_time; a = t0 + s; b = t1 + s"""
    k = height - 1 - y if from_top else y
    with np.errstate(over="ignore", invalid="ignore"):
        s = F32(k) * F32(row_time)
        return F32(t0) + s, F32(t1) + s


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bits_equal(a, b):
    return np.array_equal(bits(a), bits(b))


def params(t0, t1):
    p = host.default_params()
    p.t0, p.t1 = float(t0), float(t1)  # (float32 values: exact as doubles, and back)
    return p


def intervals(shutter, t0, t1, height=H):
    """[(a_r, b_r)] for r = 0 .. height - 1 from the library, each held to the restatement above"""
    out = []
    for r in range(height):
        a, b = device.shutter_row_interval(shutter, t0, t1, height, r)
        ra, rb = rule(t0, t1, shutter.row_time, shutter.from_top, height, r)
        assert bits(a) == bits(ra) and bits(b) == bits(rb), (r, a, b, ra, rb)
        out.append((a, b))
    return out


def bad_shutters():
    """(name, shutter, t0, t1, height, words of the message)"""
    two = host.shutter(0.01)
    two.from_top = 2
    reserved = host.shutter(0.01)
    reserved.reserved[1] = 1
    return [
        ("nan", host.shutter(float("nan")), 0.0, 1.0, 24, "row_time must be finite and >= 0"),
        ("inf", host.shutter(float("inf")), 0.0, 1.0, 24, "row_time must be finite and >= 0"),
        ("negative", host.shutter(-0.001), 0.0, 1.0, 24, "row_time must be finite and >= 0"),
        ("from_top", two, 0.0, 1.0, 24, "from_top must be 0 or 1"),
        ("reserved", reserved, 0.0, 1.0, 24, "reserved words must be 0"),
        ("overflow", host.shutter(3e37), 0.0, 1.0, 24, "readout overflows"),  # 23 * 3e37 > FLT_MAX
        ("overflow in the sum", host.shutter(1e37), 3e38, 3.1e38, 24, "readout overflows"),  # 2.3e38 + 3.1e38 > FLT_MAX
    ]
