"""Python binding of the C ABI in include/wurblpt_hip.h (libwurblpt_hip.so).

torch supplies device memory (frame buffers are torch tensors whose data_ptr() crosses the
C ABI) and streams; nothing here computes.  There is no CPU fallback: loading fails loudly
when the HIP library is missing, and rendering fails when no GPU is present."""
import ctypes as C
import os

from . import _abi

_LIB = None


def lib_path():
    # WPT_LIB_DIR: a second build of the pair of libraries (wurblpt_amd/csrc/Makefile, LIB=...), for experiments
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), os.environ.get("WPT_LIB_DIR", "lib"), "libwurblpt_hip.so")


WALK_WIDE, WALK_FULL_SHADOW, WALK_COUNT_PRODUCT, WALK_TRIANGLES_AS_GIVEN, WALK_SELECT_CORNERS, WALK_NO_FOLD, WALK_NO_BYPASS = 1, 2, 4, 8, 16, 32, 64  # wpt_set_walk (include/wurblpt_hip.h)
WALK_SMALL_WORKGROUPS = 128
WALK_HIT_DATA_IN_HBM = 256
HIT_DATA_RECORDS, HIT_DATA_HOTSPOTS, HIT_DATA_NORMALS = 1, 2, 4  # wpt_kernel_hit_data
SLICES_DECLINE_ODD = 0x100  # wpt_set_slices

EXPORTS = list(_abi.FUNCTIONS)  # every function include/wurblpt_hip.h declares (the test hooks are not among them)


def lib():
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError("%s is missing: the HIP extension must be built (python -c 'import __graft_entry__ as g; g.build()'); "
                               "there is no CPU fallback" % path)
        try:
            # the HIP runtime this process uses must be one: PyTorch ships its own libamdhip64, and when the system's copy
            # gets loaded first (this library links it) the two runtimes do not both see the device
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(path)
        # the signatures of _abi.py, one loop for all; a name the library lacks is skipped (WPT_LIB_DIR may name an older build,
        # which measurements compare with)
        for name, (restype, argtypes) in {**_abi.FUNCTIONS, **_abi.TEST_HOOK_FUNCTIONS}.items():
            fn = getattr(L, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        _LIB = L
    return _LIB


def _check(status):
    if status != _abi.WPT_OK:
        raise RuntimeError("wurblpt_hip: %s (status %d)" % (lib().wpt_last_error().decode(), status))


# ---- the wrappers' common steps ----

def _frame_size(host_scene, width, height):
    """(w, h) of a launch: the given size, or the host scene's"""
    return width or host_scene.width, height or host_scene.height


def _params(params):
    """the parameters of a launch: the given ones, or the defaults"""
    from . import host
    return params if params is not None else host.default_params()


def _stream_ptr(stream):
    return C.c_void_p(stream.cuda_stream) if stream is not None else None


def _tensor_ptr(tensor):
    return C.c_void_p(tensor.data_ptr()) if tensor is not None else None


def _array_ptr(array):
    return C.c_void_p(array.ctypes.data) if array is not None else None


COUNTER_NAMES = ("samples", "rays", "node_visits", "leaf_tests", "pdf_tests", "scatters")  # wpt_counters


def _new_counters(wanted):
    import torch
    return torch.zeros(len(COUNTER_NAMES), dtype=torch.int64, device="cuda") if wanted else None


def _counters_dict(counters):
    return dict(zip(COUNTER_NAMES, [int(x) for x in counters.cpu().tolist()]))


def shutter_row_interval(shutter, t0, t1, height, row):
    """wpt_shutter_row_interval: (a, b) as numpy float32, the exposure interval of frame row `row` (0 = bottom) of a frame of
    `height` rows exposed over [t0, t1] under host.shutter(...).  No device needed."""
    import numpy as np
    a, b = C.c_float(), C.c_float()
    _check(lib().wpt_shutter_row_interval(C.byref(shutter), float(t0), float(t1), height, row, C.cast(C.pointer(a), C.c_void_p), C.cast(C.pointer(b), C.c_void_p)))
    return np.float32(a.value), np.float32(b.value)


def shutter_span(shutter, t0, t1, height):
    """wpt_shutter_span: (first, last) as numpy float32, what the whole readout spans: a scene with moving triangles must be
    bounded for it.  No device needed."""
    import numpy as np
    first, last = C.c_float(), C.c_float()
    _check(lib().wpt_shutter_span(C.byref(shutter), float(t0), float(t1), height, C.cast(C.pointer(first), C.c_void_p), C.cast(C.pointer(last), C.c_void_p)))
    return np.float32(first.value), np.float32(last.value)


def uniform_edges(start, width, count):
    """Edges of `count` bins of one width from `start`: e_k = start + (float)k * width, each operation rounded to float32
    (no fused multiply-add), as SensorRGBTransient computes them.  Raises ValueError when they do not increase."""
    import numpy as np
    k = np.arange(count + 1, dtype=np.float32)
    edges = np.float32(start) + k * np.float32(width)
    if count < 1 or not np.all(np.isfinite(edges)) or not np.all(edges[1:] > edges[:-1]):
        raise ValueError("uniform_edges(%r, %r, %r): the edges do not increase" % (start, width, count))
    return edges


def _edges_array(edges):
    """float32 copy of a bin edge sequence (count + 1 values) for the C ABI"""
    import numpy as np
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float32))
    assert e.ndim == 1 and e.size >= 2, "bin edges: at least two values"
    return e


def _groups_table(groups, material_count):
    """uint8 copy of a light-groups table (one group per material record, or _abi.LIGHT_GROUP_NONE) for the C ABI"""
    import numpy as np
    a = np.asarray(groups)
    if a.dtype.kind not in "iub" or a.ndim != 1:
        raise TypeError("light groups: one integer per material")
    if a.size != material_count:
        raise ValueError("light groups: the table has %d entries, the scene %d materials" % (a.size, material_count))
    if a.size and (int(a.min()) < 0 or int(a.max()) > 255):
        raise ValueError("light groups: a group is a byte (0 .. 254, or %d for none)" % _abi.LIGHT_GROUP_NONE)
    return np.ascontiguousarray(a.astype(np.uint8))


def _mix_weights(weights, plane_count):
    """float32 [K, 3] of a mix's weights: an RGB triple per plane, or one number per plane for all three channels"""
    import numpy as np
    w = np.asarray(weights, dtype=np.float32)
    if w.ndim == 1:
        w = np.repeat(w[:, None], 3, axis=1)
    if w.shape != (plane_count, 3):
        raise ValueError("mix_planes: %d planes need weights [%d, 3] or [%d]" % (plane_count, plane_count, plane_count))
    return np.ascontiguousarray(w)


def mix_planes(planes, weights, out=None, stream=None):
    """wpt_postproc_mix_planes: CUDA float32 planes [K, ..., 3] (a light-groups launch's or the transient film's) mixed into one
    frame [..., 3], out[p][c] = (((0 + w[0][c] * P0[p][c]) + w[1][c] * P1[p][c]) + ...) in float32, each operation rounded on
    its own.  `weights`: [K, 3] or [K].  Asynchronous on `stream` (default: torch's current stream); returns `out`."""
    import torch
    assert planes.is_cuda and planes.is_contiguous() and planes.dtype == torch.float32 and planes.dim() >= 3 and planes.shape[-1] == 3
    K = planes.shape[0]
    w = _mix_weights(weights, K)
    if out is None:
        out = torch.empty(tuple(planes.shape[1:]), dtype=torch.float32, device=planes.device)
    pixels = planes[0].numel() // 3
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == pixels * 3
    s = stream if stream is not None else torch.cuda.current_stream()
    _check(lib().wpt_postproc_mix_planes(C.c_void_p(planes.data_ptr()), K, pixels * 3, pixels, C.c_void_p(w.ctypes.data),
                                         C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream)))
    return out


def mix_planes_host(planes, weights):
    """wpt_postproc_mix_planes_host: the same mix of numpy planes [K, ..., 3] on the CPU, bit for bit; needs no device"""
    import numpy as np
    p = np.ascontiguousarray(planes, dtype=np.float32)
    assert p.ndim >= 3 and p.shape[-1] == 3
    K = p.shape[0]
    w = _mix_weights(weights, K)
    out = np.zeros(p.shape[1:], np.float32)
    pixels = out.size // 3
    _check(lib().wpt_postproc_mix_planes_host(C.c_void_p(p.ctypes.data), K, pixels * 3, pixels, C.c_void_p(w.ctypes.data),
                                              C.c_void_p(out.ctypes.data)))
    return out


def mean_planes(planes, with_moment=False, mean_out=None, moment_out=None, stream=None):
    """wpt_postproc_mean_planes: CUDA float32 planes [K, ..., 3] (the frames of K sample streams) reduced to their mean [..., 3],
    ((P0 + P1) + ...) * (1 / float32(K)) in float32, planes in order, each operation rounded on its own; with_moment (or a
    moment_out) also the mean of their squares, the stream moment film.  Asynchronous on `stream` (default: torch's current
    stream); returns the mean, or (mean, moment)."""
    import torch
    assert planes.is_cuda and planes.is_contiguous() and planes.dtype == torch.float32 and planes.dim() >= 3 and planes.shape[-1] == 3
    K = planes.shape[0]
    if K == 0:
        raise ValueError("mean_planes: no planes")
    if mean_out is None:
        mean_out = torch.empty(tuple(planes.shape[1:]), dtype=torch.float32, device=planes.device)
    if moment_out is None and with_moment:
        moment_out = torch.empty(tuple(planes.shape[1:]), dtype=torch.float32, device=planes.device)
    pixels = planes[0].numel() // 3
    for t in (mean_out, moment_out):
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == pixels * 3)
    s = stream if stream is not None else torch.cuda.current_stream()
    _check(lib().wpt_postproc_mean_planes(C.c_void_p(planes.data_ptr()), K, pixels * 3, pixels, C.c_void_p(mean_out.data_ptr()),
                                          _tensor_ptr(moment_out), C.c_void_p(s.cuda_stream)))
    return (mean_out, moment_out) if moment_out is not None else mean_out


def mean_planes_host(planes, with_moment=False):
    """wpt_postproc_mean_planes_host: the same mean (and moment) of numpy planes [K, ..., 3] on the CPU, bit for bit; needs no device"""
    import numpy as np
    p = np.ascontiguousarray(planes, dtype=np.float32)
    assert p.ndim >= 3 and p.shape[-1] == 3
    K = p.shape[0]
    mean = np.zeros(p.shape[1:], np.float32)
    moment = np.zeros(p.shape[1:], np.float32) if with_moment else None
    pixels = mean.size // 3
    _check(lib().wpt_postproc_mean_planes_host(C.c_void_p(p.ctypes.data), K, pixels * 3, pixels, C.c_void_p(mean.ctypes.data),
                                               _array_ptr(moment)))
    return (mean, moment) if with_moment else mean


def merge_means(a, count_a, b, count_b, out=None, stream=None):
    """wpt_postproc_merge_means: two CUDA float32 results of one shape (frames or moment films), `a` over count_a sample streams
    and `b` over count_b others, merged into the result of count_a + count_b streams:
    (float32(count_a) * a + float32(count_b) * b) / float32(count_a + count_b), each operation rounded on its own.  `out` may be
    `a` or `b`.  Asynchronous on `stream` (default: torch's current stream); returns `out`."""
    import torch
    for t in (a, b):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
    assert a.shape == b.shape, "merge_means: results of one shape"
    if out is None:
        out = torch.empty_like(a)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == a.numel()
    s = stream if stream is not None else torch.cuda.current_stream()
    _check(lib().wpt_postproc_merge_means(C.c_void_p(a.data_ptr()), int(count_a), C.c_void_p(b.data_ptr()), int(count_b), a.numel(),
                                          C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream)))
    return out


def merge_means_host(a, count_a, b, count_b):
    """wpt_postproc_merge_means_host: the same merge of numpy arrays on the CPU, bit for bit; needs no device"""
    import numpy as np
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, "merge_means: results of one shape"
    out = np.zeros(a.shape, np.float32)
    _check(lib().wpt_postproc_merge_means_host(C.c_void_p(a.ctypes.data), int(count_a), C.c_void_p(b.ctypes.data), int(count_b), a.size,
                                               C.c_void_p(out.ctypes.data)))
    return out


def device_lanes(device=None):
    """wpt_device_lanes: compute units * 1024 of HIP device `device` (None: the current one)"""
    if device is None:
        current = C.c_int(0)
        _check(lib().wpt_current_device(C.byref(current)))
        device = current.value
    lanes = C.c_uint32(0)
    _check(lib().wpt_device_lanes(int(device), C.byref(lanes)))
    return int(lanes.value)


def split_plan(pixels, samples_sqrt, lanes=None):
    """wpt_split_plan: (stream_count, stream_samples_sqrt) a frame of `pixels` pixels and samples_sqrt^2 samples per pixel is split
    into for a device that holds `lanes` lanes (None: device_lanes() of the current device); stream_count is a square and
    stream_count * stream_samples_sqrt^2 == samples_sqrt^2.  With `lanes` given it needs no device."""
    if lanes is None:
        lanes = device_lanes()
    for name, v, top in (("pixels", pixels, 2 ** 64), ("samples_sqrt", samples_sqrt, 2 ** 32), ("lanes", lanes, 2 ** 32)):
        if not 0 <= int(v) < top:
            raise ValueError("split_plan: %s out of range" % name)
    count, sqrt = C.c_uint32(0), C.c_uint32(0)
    _check(lib().wpt_split_plan(int(pixels), int(samples_sqrt), int(lanes), C.byref(count), C.byref(sqrt)))
    return int(count.value), int(sqrt.value)


GUIDE_NAMES = ("camera_space_positions", "camera_space_material_normals", "materials")  # the ground truth arrays a denoiser call reads


def _denoise_guide(guide):
    """(P, n, m) of a denoiser call: a dict as ground_truth / ground_truth_device return it, or the three arrays"""
    if isinstance(guide, dict):
        return tuple(guide[name] for name in GUIDE_NAMES)
    P, n, m = guide
    return P, n, m


def denoise_form(step):
    """wpt_postproc_denoise_form: "tile" or "gather", the form the device's iteration with this step takes"""
    return lib().wpt_postproc_denoise_form(int(step)).decode()


def _denoise_inputs(frame, moments, samples_sqrt, guide, colours, stream):
    """The input side of a denoiser call, shared with temporal_accumulate: the checked input tensors in the order of the C
    parameters (the map as 16-bit words among them), w, h and the launch stream, ordered behind the work on torch's current
    stream.  Nothing is allocated but the map's 16-bit copy, where one is needed."""
    import numpy as np
    import torch
    h, w = int(frame.shape[0]), int(frame.shape[1])
    P, n, m = _denoise_guide(guide)
    for t, what in ((frame, "frame"), (moments, "moments"), (P, "positions"), (n, "normals")) + tuple(zip(colours, ("albedo", "emission"))):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == (h, w, 3), "denoise: %s must be CUDA float32 [h, w, 3]" % what
    assert m.is_cuda and m.is_contiguous() and m.dtype == torch.int32 and m.numel() == w * h, "denoise: materials must be CUDA int32 [h, w]"
    if isinstance(samples_sqrt, (int, np.integer)):
        if not 0 <= int(samples_sqrt) <= 65535:
            raise ValueError("the sample count's square root must lie in [0, 65535]")
        samples_sqrt = np.full((h, w), int(samples_sqrt), np.uint16)
    elif not (isinstance(samples_sqrt, torch.Tensor) and samples_sqrt.is_cuda):
        _map_int(samples_sqrt)
    assert tuple(samples_sqrt.shape) == (h, w), "samples_sqrt: [h, w]"
    current = torch.cuda.current_stream()
    launch = stream if stream is not None else current
    m16 = _map_u16_device(samples_sqrt)
    if launch != current:
        launch.wait_stream(current)
        m16.record_stream(launch)
    return (frame, moments, m16, P, n, m) + tuple(colours), w, h, launch


def _launch_outputs(launch, *tensors):
    """new output tensors of a launch on a stream that is not torch's current one: theirs to keep until that stream has passed"""
    import torch
    if launch != torch.cuda.current_stream():
        for t in tensors:
            if t is not None:
                t.record_stream(launch)


def _denoise_args(frame, moments, samples_sqrt, guide, colours, params, variance_out, stream):
    """What denoise (colours = ()) and denoise_demodulated (colours = (albedo, emission)) hand to the library: _denoise_inputs,
    the parameters and the new output tensors."""
    import torch
    inputs, w, h, launch = _denoise_inputs(frame, moments, samples_sqrt, guide, colours, stream)
    out = torch.empty((h, w, 3), dtype=torch.float32, device=frame.device)
    variance = torch.empty((h, w), dtype=torch.float32, device=frame.device) if variance_out else None
    _launch_outputs(launch, out, variance)
    return inputs, w, h, params if params is not None else _abi.DenoiseParams(), out, variance, launch


def _denoise_host_args(frame, moments, samples_sqrt, guide, colours, params, variance_out):
    """_denoise_args for the host forms: float32 / int32 numpy copies, the map as uint16, zeroed outputs"""
    import numpy as np
    f = np.ascontiguousarray(frame, dtype=np.float32)
    assert f.ndim == 3 and f.shape[2] == 3, "denoise: the frame must be [h, w, 3]"
    h, w = f.shape[:2]
    P, n, m = _denoise_guide(guide)
    mo, P, n, *colours = (np.ascontiguousarray(a, dtype=np.float32) for a in (moments, P, n) + tuple(colours))
    m = np.ascontiguousarray(m, dtype=np.int32)
    assert all(a.shape == f.shape for a in [mo, P, n] + colours) and m.size == w * h, "denoise: arrays of the frame's size"
    if isinstance(samples_sqrt, (int, np.integer)):
        samples_sqrt = np.full((h, w), int(samples_sqrt), np.int64)
    a = _map_int(samples_sqrt)
    assert a.shape == (h, w), "samples_sqrt: [h, w]"
    m16 = np.ascontiguousarray(a.astype(np.uint16))
    out = np.zeros((h, w, 3), np.float32)
    variance = np.zeros((h, w), np.float32) if variance_out else None
    return [f, mo, m16, P, n, m] + colours, w, h, params if params is not None else _abi.DenoiseParams(), out, variance


def denoise(frame, moments, samples_sqrt, guide, params=None, variance_out=False, stream=None):
    """wpt_postproc_denoise: the edge-avoiding a-trous filter with variance guidance (include/wurblpt_hip.h has the formula) on
    CUDA tensors.  `frame`, `moments`: float32 [h, w, 3] (an adaptive render's frame and moment film); `samples_sqrt`: the map the
    frame was rendered with (any integer tensor or array [h, w]) or one integer for all pixels; `guide`: the dict of
    DeviceScene.ground_truth_device (GUIDE_NAMES) or the tuple (positions, normals, materials); `params`: _abi.DenoiseParams
    (None: the defaults).  Asynchronous on `stream` (None: torch's current stream), ordered behind the work on the current
    stream.  Returns the filtered frame, and with variance_out the variance of its luminance [h, w] as well."""
    inputs, w, h, p, out, variance, launch = _denoise_args(frame, moments, samples_sqrt, guide, (), params, variance_out, stream)
    _check(lib().wpt_postproc_denoise(*[_tensor_ptr(t) for t in inputs], w, h, C.byref(p), _tensor_ptr(out), _tensor_ptr(variance),
                                      _stream_ptr(launch)))
    return (out, variance) if variance_out else out


def denoise_host(frame, moments, samples_sqrt, guide, params=None, variance_out=False):
    """wpt_postproc_denoise_host: the same filter of numpy arrays on the CPU, bit for bit; needs no device"""
    inputs, w, h, p, out, variance = _denoise_host_args(frame, moments, samples_sqrt, guide, (), params, variance_out)
    _check(lib().wpt_postproc_denoise_host(*[_array_ptr(a) for a in inputs], w, h, C.byref(p), _array_ptr(out), _array_ptr(variance)))
    return (out, variance) if variance_out else out


def denoise_demodulated(frame, moments, samples_sqrt, guide, albedo=None, emission=None, params=None, albedo_floor=0.0, variance_out=False,
                        stream=None):
    """wpt_postproc_denoise_demodulated: denoise() on (frame - emission) / albedo, the surface's own colours put back afterwards
    (include/wurblpt_hip.h has the rule).  `albedo`, `emission`: CUDA float32 [h, w, 3]; None: the entries "albedo" and
    "emission" of `guide`, the dict of DeviceScene.first_hit_colours_device.  `albedo_floor` <= 0: the default 1 / 64.  With
    variance_out the variance of the DEMODULATED luminance [h, w] is returned as well.  Everything else as for denoise()."""
    colours = (guide["albedo"] if albedo is None else albedo, guide["emission"] if emission is None else emission)
    inputs, w, h, p, out, variance, launch = _denoise_args(frame, moments, samples_sqrt, guide, colours, params, variance_out, stream)
    _check(lib().wpt_postproc_denoise_demodulated(*[_tensor_ptr(t) for t in inputs], w, h, C.byref(p), float(albedo_floor), _tensor_ptr(out),
                                                  _tensor_ptr(variance), _stream_ptr(launch)))
    return (out, variance) if variance_out else out


def denoise_demodulated_host(frame, moments, samples_sqrt, guide, albedo=None, emission=None, params=None, albedo_floor=0.0,
                             variance_out=False):
    """wpt_postproc_denoise_demodulated_host: the same of numpy arrays on the CPU, bit for bit; needs no device"""
    colours = (guide["albedo"] if albedo is None else albedo, guide["emission"] if emission is None else emission)
    inputs, w, h, p, out, variance = _denoise_host_args(frame, moments, samples_sqrt, guide, colours, params, variance_out)
    _check(lib().wpt_postproc_denoise_demodulated_host(*[_array_ptr(a) for a in inputs], w, h, C.byref(p), float(albedo_floor),
                                                       _array_ptr(out), _array_ptr(variance)))
    return (out, variance) if variance_out else out


MOTION_NAMES = ("pixel_space_offset_to_prev", "camera_space_offset_to_prev")  # the ground truth arrays temporal accumulation follows


def temporal_params(max_history=32.0, normal_cos_min=0.9, position_tolerance=0.02):
    """wpt_temporal_params with the header's defaults"""
    return _abi.TemporalParams(max_history, normal_cos_min, position_tolerance)


def _motion(motion):
    """(pixel offsets, camera offsets) of a temporal call: a dict with MOTION_NAMES (as ground_truth / ground_truth_device return
    it), the two arrays, or None for a scene and a camera at rest"""
    if motion is None:
        return None, None
    if isinstance(motion, dict):
        return tuple(motion[name] for name in MOTION_NAMES)
    pixel, camera = motion
    return pixel, camera


def temporal_accumulate(frame, moments, samples_sqrt, guide, motion=None, history=None, params=None, length_out=False, stream=None):
    """wpt_postproc_temporal_accumulate: the current frame and the previous history into a new history (include/wurblpt_hip.h has
    the rule and the layout) on CUDA tensors.  `frame`, `moments`, `samples_sqrt`, `guide`: as for denoise(), the dicts of
    ground_truth_device and first_hit_colours_device included; `motion`: a dict with MOTION_NAMES (float32 [h, w, 2] and
    [h, w, 3]) or None for a scene and a camera at rest; `history`: the previous call's result, None for the first frame (it is
    read, never written); `params`: temporal_params() (None: the defaults).  Asynchronous on `stream` (None: torch's current
    stream), ordered behind the work on the current stream; as with denoise(), the caller keeps the inputs -- `history` and the
    offsets among them -- alive and unchanged until that stream has passed the call.  Returns the new history, a float32 tensor
    [3, h, w, 4], and with length_out the history length per pixel [h, w] as well."""
    import torch
    inputs, w, h, launch = _denoise_inputs(frame, moments, samples_sqrt, guide, (), stream)
    pixel, camera = _motion(motion)
    for t, comps, what in ((pixel, 2, MOTION_NAMES[0]), (camera, 3, MOTION_NAMES[1])):
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == (h, w, comps)), \
            "temporal_accumulate: %s must be CUDA float32 [h, w, %d]" % (what, comps)
    assert history is None or (history.is_cuda and history.is_contiguous() and history.dtype == torch.float32
                               and tuple(history.shape) == (3, h, w, 4)), "temporal_accumulate: the history must be CUDA float32 [3, h, w, 4]"
    out = torch.empty((3, h, w, 4), dtype=torch.float32, device=frame.device)
    length = torch.empty((h, w), dtype=torch.float32, device=frame.device) if length_out else None
    _launch_outputs(launch, out, length)
    p = params if params is not None else _abi.TemporalParams()
    _check(lib().wpt_postproc_temporal_accumulate(*[_tensor_ptr(t) for t in inputs], _tensor_ptr(pixel), _tensor_ptr(camera), _tensor_ptr(history),
                                                  w, h, C.byref(p), _tensor_ptr(out), _tensor_ptr(length), _stream_ptr(launch)))
    return (out, length) if length_out else out


def temporal_accumulate_host(frame, moments, samples_sqrt, guide, motion=None, history=None, params=None, length_out=False):
    """wpt_postproc_temporal_accumulate_host: the same of numpy arrays on the CPU, bit for bit; needs no device"""
    import numpy as np
    inputs, w, h, _, _, _ = _denoise_host_args(frame, moments, samples_sqrt, guide, (), None, False)
    pixel, camera = (None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in _motion(motion))
    assert (pixel is None or pixel.shape == (h, w, 2)) and (camera is None or camera.shape == (h, w, 3)), "temporal_accumulate: offsets [h, w, 2] and [h, w, 3]"
    if history is not None:
        history = np.ascontiguousarray(history, dtype=np.float32)
        assert history.shape == (3, h, w, 4), "temporal_accumulate: the history must be [3, h, w, 4]"
    out = np.zeros((3, h, w, 4), np.float32)
    length = np.zeros((h, w), np.float32) if length_out else None
    p = params if params is not None else _abi.TemporalParams()
    _check(lib().wpt_postproc_temporal_accumulate_host(*[_array_ptr(a) for a in inputs], _array_ptr(pixel), _array_ptr(camera), _array_ptr(history),
                                                       w, h, C.byref(p), _array_ptr(out), _array_ptr(length)))
    return (out, length) if length_out else out


def denoise_history(history, params=None, variance_out=False, stream=None):
    """wpt_postproc_denoise_history: denoise()'s iterations on a history of temporal_accumulate (CUDA float32 [3, h, w, 4]), which
    is not written.  `params`: _abi.DenoiseParams (None: the defaults); iterations=0 returns the accumulated frame and its
    variance.  Asynchronous on `stream` as denoise() is.  Returns the frame [h, w, 3], and with variance_out the variance of its
    luminance [h, w] as well."""
    import torch
    assert history.is_cuda and history.is_contiguous() and history.dtype == torch.float32 and history.dim() == 4 \
        and history.shape[0] == 3 and history.shape[3] == 4, "denoise_history: the history must be CUDA float32 [3, h, w, 4]"
    h, w = int(history.shape[1]), int(history.shape[2])
    current = torch.cuda.current_stream()
    launch = stream if stream is not None else current
    out = torch.empty((h, w, 3), dtype=torch.float32, device=history.device)
    variance = torch.empty((h, w), dtype=torch.float32, device=history.device) if variance_out else None
    if launch != current:
        launch.wait_stream(current)
    _launch_outputs(launch, out, variance)
    p = params if params is not None else _abi.DenoiseParams()
    _check(lib().wpt_postproc_denoise_history(_tensor_ptr(history), w, h, C.byref(p), _tensor_ptr(out), _tensor_ptr(variance), _stream_ptr(launch)))
    return (out, variance) if variance_out else out


def denoise_history_host(history, params=None, variance_out=False):
    """wpt_postproc_denoise_history_host: the same of a numpy history on the CPU, bit for bit; needs no device"""
    import numpy as np
    history = np.ascontiguousarray(history, dtype=np.float32)
    assert history.ndim == 4 and history.shape[0] == 3 and history.shape[3] == 4, "denoise_history: the history must be [3, h, w, 4]"
    h, w = history.shape[1:3]
    out = np.zeros((h, w, 3), np.float32)
    variance = np.zeros((h, w), np.float32) if variance_out else None
    p = params if params is not None else _abi.DenoiseParams()
    _check(lib().wpt_postproc_denoise_history_host(_array_ptr(history), w, h, C.byref(p), _array_ptr(out), _array_ptr(variance)))
    return (out, variance) if variance_out else out


def _image_tensor(image, what):
    """(h, w, c) of a CUDA float32 image [h, w, c] or [h, w]"""
    import torch
    assert image.is_cuda and image.is_contiguous() and image.dtype == torch.float32 and image.dim() in (2, 3), "%s: a CUDA float32 image [h, w, c]" % what
    return int(image.shape[0]), int(image.shape[1]), int(image.shape[2]) if image.dim() == 3 else 1


def _image_array(image, what):
    """a float32 numpy image [h, w, c] (from [h, w, c] or [h, w]) and its (h, w, c)"""
    import numpy as np
    a = np.ascontiguousarray(image, dtype=np.float32)
    assert a.ndim in (2, 3), "%s: an image [h, w, c]" % what
    if a.ndim == 2:
        a = a[:, :, None]
    return a, a.shape


def _image_launch(image, out_shape, stream):
    """the output tensor of an image operation and the stream it is launched on, ordered behind the current stream's work"""
    import torch
    out = torch.empty(out_shape, dtype=torch.float32, device=image.device)
    current = torch.cuda.current_stream()
    launch = stream if stream is not None else current
    if launch != current:
        launch.wait_stream(current)
        out.record_stream(launch)
        image.record_stream(launch)
    return out, launch


def image_ops_tile():
    """wpt_postproc_image_ops_tile: (width, height) of the output pixels of one workgroup of the device forms below"""
    w, h = C.c_uint32(0), C.c_uint32(0)
    lib().wpt_postproc_image_ops_tile(C.byref(w), C.byref(h))
    return int(w.value), int(h.value)


def despeckle_form():
    """wpt_postproc_despeckle_form: "tile" or "gather", the form the device's despeckle takes"""
    return lib().wpt_postproc_despeckle_form().decode()


def set_despeckle_form(form):
    """wpt_set_despeckle_form: -1 the form the library was built with, 0 gather, 1 tile (process-global; for tests and measurements)"""
    _check(lib().wpt_set_despeckle_form(int(form)))


def resample(image, new_width, new_height, stream=None):
    """wpt_postproc_resample (scale() of the reference): a CUDA float32 image [h, w, c], c in 1 .. 4, row 0 at the bottom,
    resampled bilinearly to [new_height, new_width, c].  Asynchronous on `stream` (None: torch's current stream)."""
    h, w, c = _image_tensor(image, "resample")
    out, launch = _image_launch(image, (int(new_height), int(new_width), c) if image.dim() == 3 else (int(new_height), int(new_width)), stream)
    _check(lib().wpt_postproc_resample(C.c_void_p(image.data_ptr()), w, h, c, int(new_width), int(new_height), C.c_void_p(out.data_ptr()),
                                       C.c_void_p(launch.cuda_stream)))
    return out


def resample_host(image, new_width, new_height):
    """wpt_postproc_resample_host: the same on a numpy image on the CPU, bit for bit; needs no device"""
    import numpy as np
    a, (h, w, c) = _image_array(image, "resample")
    out = np.zeros((int(new_height), int(new_width), c), np.float32)
    _check(lib().wpt_postproc_resample_host(C.c_void_p(a.ctypes.data), w, h, c, int(new_width), int(new_height), C.c_void_p(out.ctypes.data)))
    return out


def lens_warp(image, camera, forward, stream=None):
    """wpt_postproc_lens_warp (applyLensDistortion() of the reference): a CUDA float32 image [h, w, c] through the lens of `camera`
    (an _abi.Camera, e.g. host.lens_camera(...) or a scene's; only its distortion part is read).  forward: an undistorted render
    becomes what the lens shows (distort()); otherwise a distorted image is rectified (undistort())."""
    h, w, c = _image_tensor(image, "lens_warp")
    out, launch = _image_launch(image, tuple(image.shape), stream)
    _check(lib().wpt_postproc_lens_warp(C.c_void_p(image.data_ptr()), w, h, c, C.byref(camera), 1 if forward else 0, C.c_void_p(out.data_ptr()),
                                        C.c_void_p(launch.cuda_stream)))
    return out


def lens_warp_host(image, camera, forward):
    """wpt_postproc_lens_warp_host: the same on a numpy image on the CPU, bit for bit; needs no device"""
    import numpy as np
    a, (h, w, c) = _image_array(image, "lens_warp")
    out = np.zeros((h, w, c), np.float32)
    _check(lib().wpt_postproc_lens_warp_host(C.c_void_p(a.ctypes.data), w, h, c, C.byref(camera), 1 if forward else 0, C.c_void_p(out.ctypes.data)))
    return out


def despeckle(image, min_factor=1.25, stream=None):
    """wpt_postproc_despeckle (despeckle() of the reference, the firefly filter): a CUDA float32 RGB image [h, w, 3]; a pixel whose
    luminance is the greatest of its 3 x 3 neighbourhood and at least min_factor times the second greatest becomes the
    neighbourhood's median pixel.  The values must be finite."""
    h, w, c = _image_tensor(image, "despeckle")
    out, launch = _image_launch(image, tuple(image.shape), stream)
    _check(lib().wpt_postproc_despeckle(C.c_void_p(image.data_ptr()), w, h, c, float(min_factor), C.c_void_p(out.data_ptr()),
                                        C.c_void_p(launch.cuda_stream)))
    return out


def despeckle_host(image, min_factor=1.25):
    """wpt_postproc_despeckle_host: the same on a numpy image on the CPU, bit for bit; needs no device"""
    import numpy as np
    a, (h, w, c) = _image_array(image, "despeckle")
    out = np.zeros((h, w, c), np.float32)
    _check(lib().wpt_postproc_despeckle_host(C.c_void_p(a.ctypes.data), w, h, c, float(min_factor), C.c_void_p(out.ctypes.data)))
    return out


def distance_to_coords(distances, camera, pmd_space=False, stream=None):
    """wpt_postproc_distance_to_coords (cameraSpaceDistanceToCoords() of the reference, and with pmd_space cameraSpaceToPMDSpace()
    behind it): CUDA float32 distances [h, w] or [h, w, c] (component 0 is the distance from the camera, as the ToF sensor's result
    and the ground truth's camera_space_distances hold it) to coordinates [h, w, 3]: (x, y, -z) in camera space, or (x, -y, z) in
    the PMD camera's space.  `camera`: an _abi.Camera; its dist_center, dist_inverse_focal_length and lens are read."""
    h, w, c = _image_tensor(distances, "distance_to_coords")
    out, launch = _image_launch(distances, (h, w, 3), stream)
    _check(lib().wpt_postproc_distance_to_coords(C.c_void_p(distances.data_ptr()), w, h, c, C.byref(camera), 1 if pmd_space else 0,
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(launch.cuda_stream)))
    return out


def distance_to_coords_host(distances, camera, pmd_space=False):
    """wpt_postproc_distance_to_coords_host: the same on a numpy image on the CPU, bit for bit; needs no device"""
    import numpy as np
    a, (h, w, c) = _image_array(distances, "distance_to_coords")
    out = np.zeros((h, w, 3), np.float32)
    _check(lib().wpt_postproc_distance_to_coords_host(C.c_void_p(a.ctypes.data), w, h, c, C.byref(camera), 1 if pmd_space else 0,
                                                      C.c_void_p(out.ctypes.data)))
    return out


def _map_int(samples_sqrt):
    """the integer values of a sample-count map, checked to lie in [0, 65535]"""
    import numpy as np
    a = samples_sqrt.detach().cpu().numpy() if hasattr(samples_sqrt, "detach") else np.asarray(samples_sqrt)
    if a.dtype.kind not in "iub":
        raise TypeError("the sample-count map must hold integers, not %s" % a.dtype)
    if a.size and (int(a.min()) < 0 or int(a.max()) > 65535):
        raise ValueError("the sample-count map's values must lie in [0, 65535]")
    return a


def _map_u16_device(samples_sqrt):
    """the map as 16-bit words in a CUDA tensor (uint16 bits), made on torch's current stream.  A host map has been checked by
    _map_int already and is uploaded; a CUDA map of torch.uint16 is used as it is (every value is valid: no check, no host round
    trip); any other CUDA integer map is checked on the device, and only the one flag of that check is read back."""
    import numpy as np
    import torch
    if not (isinstance(samples_sqrt, torch.Tensor) and samples_sqrt.is_cuda):
        a = np.ascontiguousarray(np.asarray(samples_sqrt).astype(np.uint16))
        return torch.from_numpy(a.view(np.int16)).to("cuda")
    t = samples_sqrt.detach()
    if t.dtype == torch.uint16:
        return t.contiguous()
    if t.dtype.is_floating_point or t.dtype.is_complex:
        raise TypeError("the sample-count map must hold integers, not %s" % t.dtype)
    t = t.to(torch.int32)
    if bool(((t < 0) | (t > 65535)).any()):
        raise ValueError("the sample-count map's values must lie in [0, 65535]")
    return torch.where(t >= 32768, t - 65536, t).to(torch.int16).contiguous()


def samples_sqrt_for_error(frame, moments, pilot_samples_sqrt, rel_error, min_sqrt, max_sqrt, floor):
    """A sample-count map (numpy uint16 [h, w]) from a pilot render with pilot_samples_sqrt^2 samples and its moment film:
    per pixel, in float64, N0 = pilot^2; var_c = max(m_c - f_c^2, 0) * (N0 / (N0 - 1));
    need = max over c of var_c / (rel_error^2 * max(|f_c|, floor)^2); n = clamp(ceil(sqrt(need)), min_sqrt, max_sqrt).
    A pixel with a non-finite input or need gets max_sqrt.  The C++ samplesSqrtForError (include/wurblpt/wurblpt.hpp), value
    for value; its refusals are ValueError here."""
    import numpy as np
    f = frame.detach().cpu().numpy() if hasattr(frame, "detach") else np.asarray(frame)
    m = moments.detach().cpu().numpy() if hasattr(moments, "detach") else np.asarray(moments)
    if int(pilot_samples_sqrt) < 2:
        raise ValueError("samples_sqrt_for_error: the pilot needs pilot_samples_sqrt >= 2")
    if f.shape != m.shape or f.ndim != 3 or f.shape[2] != 3:
        raise ValueError("samples_sqrt_for_error: frame and moments must be arrays [h, w, 3] of one shape")
    rel_error, floor = float(rel_error), float(floor)
    if not rel_error > 0.0 or not floor >= 0.0 or not 0 <= int(min_sqrt) <= int(max_sqrt) <= 65535:
        raise ValueError("samples_sqrt_for_error: needs rel_error > 0, floor >= 0 and min_sqrt <= max_sqrt <= 65535")
    f = f.astype(np.float64)
    m = m.astype(np.float64)
    n0 = float(pilot_samples_sqrt) * float(pilot_samples_sqrt)
    scale = n0 / (n0 - 1.0)
    r2 = rel_error * rel_error
    with np.errstate(all="ignore"):
        var = np.maximum(m - f * f, 0.0) * scale
        d = np.maximum(np.abs(f), floor)
        q = var / (r2 * (d * d))
    finite = np.isfinite(f).all(axis=2) & np.isfinite(m).all(axis=2) & np.isfinite(q).all(axis=2)
    need = np.where(finite[..., None], q, 0.0).max(axis=2)
    n = np.clip(np.ceil(np.sqrt(need)), float(min_sqrt), float(max_sqrt))
    n[~finite] = max_sqrt
    return n.astype(np.uint16)


def _tof_phases(sensor, phases):
    """the sensor record of a launch: all of `sensor`'s phase images, or those whose indices `phases` lists (in that order)"""
    if phases is None:
        return sensor
    s = _abi.TofSensor.from_buffer_copy(sensor)
    phases = list(phases)
    if not (1 <= len(phases) <= _abi.TOF_MAX_PHASES and all(0 <= j < sensor.phase_count for j in phases)):
        raise ValueError("phases: 1 to %d indices below the sensor's phase count %d" % (_abi.TOF_MAX_PHASES, sensor.phase_count))
    s.phase_count = len(phases)
    for k, j in enumerate(phases):
        s.tau[k] = sensor.tau[j]
    return s


def tof_accumulate_host(sensor, phase, radiance_w, opl_w, is_tof_light, acc):
    """wpt_tof_accumulate_host: one contribution added to acc = float32[3] (a, b, total) on the CPU by the kernels' code"""
    _check(lib().wpt_tof_accumulate_host(C.byref(sensor), phase, radiance_w, opl_w, 1 if is_tof_light else 0, C.c_void_p(acc.ctypes.data)))
    return acc


def tof_result(phase_differences, modulation_frequency):
    """SensorTofAmcw::result() (sensor_tof_amcw.hpp:173-213) in numpy float32.  `phase_differences`: [n, ...] with n a multiple
    of 4, a - b of the n phase images (digital numbers or energies: distance and phase shift do not depend on their scale,
    amplitude and intensity scale with it).  Returns (distance [m], amplitude, intensity, phase_shift [rad])."""
    import numpy as np
    from . import host
    D = np.asarray(phase_differences, dtype=np.float32)
    n = D.shape[0]
    assert n % 4 == 0 and n > 0, "a multiple of 4 phase images"
    d0, d1, d2, d3 = D[0], D[n // 4], D[2 * n // 4], D[3 * n // 4]
    re, im = d0 - d2, d3 - d1
    zero = (np.abs(d0 - d2) <= 0) & (np.abs(d1 - d3) <= 0)
    # the C library's atan2f, which the reference's std::atan2 is (numpy's own float32 arctan2 differs from it in the last bit)
    atan2f = C.CFUNCTYPE(C.c_float, C.c_float, C.c_float)(("atan2f", C.CDLL("libm.so.6")))
    shift = np.frompyfunc(atan2f, 2, 1)(im, re).astype(np.float32)
    # `phaseShift += 2.0 * pi` with the float pi: a double addition rounded to float
    shift = np.where(shift < 0, (shift.astype(np.float64) + 2.0 * float(np.float32(np.pi))).astype(np.float32), shift)
    frac_c_modfreq = np.float32(host.SPEED_OF_LIGHT / float(modulation_frequency))
    distance = frac_c_modfreq * shift * np.float32(0.25) * np.float32(1.0 / np.pi)
    shift = np.where(zero, np.float32(0), shift).astype(np.float32)
    distance = np.where(zero, np.float32(0), distance).astype(np.float32)
    amplitude = (np.sqrt((d0 - d2) * (d0 - d2) + (d1 - d3) * (d1 - d3)) * np.float32(np.pi / 2)).astype(np.float32)
    intensity = (np.float32(0.5) * (d0 + d1 + d2 + d3)).astype(np.float32)
    return distance, amplitude, intensity, shift


def device_count():
    return lib().wpt_device_count()


def set_slices(n):
    """wpt_set_slices: 0 = the library's plan, 1 = never, 2 .. 15 = that many units per pixel (| SLICES_DECLINE_ODD: tests)"""
    _check(lib().wpt_set_slices(n))


def slices_plan(block_size, lanes_at_once, samples_sqrt):
    """wpt_slices_plan: (units, rows) the library cuts the pixels of such a launch into; needs no device"""
    units, rows = C.c_uint32(), C.c_uint32()
    _check(lib().wpt_slices_plan(block_size, lanes_at_once, samples_sqrt, C.byref(units), C.byref(rows)))
    return int(units.value), int(rows.value)


SENSOR_FRAME, SENSOR_TRANSIENT, SENSOR_VIEWS, SENSOR_ADAPTIVE, SENSOR_TOF = range(5)  # wpt_kernel_choice


def kernel_choice(need, sensor, count, node_count, tri_count, material_count, scene_has_wide=False, variant=0, walk=0):
    """wpt_kernel_choice: (name, form, (F, count, ldsScene, wide), sceneLdsBytes, materialsInLds) of the kernel the library would
    launch; needs no device"""
    name, form, key, lds_bytes, materials = C.c_char_p(), C.c_char_p(), (C.c_uint32 * 4)(), C.c_uint64(), C.c_uint32()
    _check(lib().wpt_kernel_choice(need, sensor, int(count), node_count, tri_count, material_count, int(scene_has_wide), variant, walk,
                                   C.byref(name), C.byref(form), key, C.byref(lds_bytes), C.byref(materials)))
    return name.value.decode(), form.value.decode(), (key[0], bool(key[1]), bool(key[2]), bool(key[3])), int(lds_bytes.value), int(materials.value)


def kernel_table():
    """wpt_kernel_table_entry: [((F, count, ldsScene, wide), name)] of every kernel the library has"""
    rows = []
    key, name = (C.c_uint32 * 4)(), C.c_char_p()
    while lib().wpt_kernel_table_entry(len(rows), key, C.byref(name)) == _abi.WPT_OK:
        rows.append(((key[0], bool(key[1]), bool(key[2]), bool(key[3])), name.value.decode()))
    return rows


STRATEGIES = ("one pass", "two passes", "adaptive order", "sliced")  # WPT_STRATEGY_*
PLAN_WORDS = ("wavefront", "wavefront_falls_back", "pooled", "strategy", "units", "rows", "passes")  # WPT_PLAN_*, WPT_PLAN_WORDS of them


def launch_plan(sensor, count, need, scene_in_lds, block_size, samples_sqrt, cu_count, variant=0, wavefront_mode=0, slices=0):
    """wpt_launch_plan: which passes render such a launch, as a dict: wavefront, wavefront_falls_back, pooled (bools), strategy (one of
    STRATEGIES), units, rows, passes; needs no device"""
    w = (C.c_uint32 * len(PLAN_WORDS))()
    _check(lib().wpt_launch_plan(*[int(v) for v in (sensor, count, need, scene_in_lds, block_size, samples_sqrt, cu_count, variant, wavefront_mode,
                                                    slices)], w))
    plan = dict(zip(PLAN_WORDS, (int(v) for v in w)))
    for k in ("wavefront", "wavefront_falls_back", "pooled"):
        plan[k] = bool(plan[k])
    plan["strategy"] = STRATEGIES[plan["strategy"]]
    return plan


def last_slice_stats():
    """wpt_last_slice_stats: (taken, continued) of the most recent render call; waits for the device"""
    taken, continued = C.c_uint64(), C.c_uint64()
    _check(lib().wpt_last_slice_stats(C.byref(taken), C.byref(continued)))
    return int(taken.value), int(continued.value)


def kernel_workgroup():
    """wpt_kernel_workgroup: (lanes per workgroup, ordered boxes) of the most recent render call's path-tracing kernel"""
    ordered = C.c_uint32()
    lanes = lib().wpt_kernel_workgroup(C.byref(ordered))
    return int(lanes), bool(ordered.value)


def kernel_hit_data():
    """wpt_kernel_hit_data: the parts of a hit's data (HIT_DATA_*) the most recent render call's kernel read from LDS"""
    return int(lib().wpt_kernel_hit_data())


def kernel_materials_in_lds():
    """wpt_kernel_materials_in_lds: did the most recent render call's kernel read the material records by LDS address?"""
    return bool(lib().wpt_kernel_materials_in_lds())


def kernel_launch_record():
    """wpt_kernel_launch_record: did the most recent render call's kernel read the launch's constants from a record in LDS?"""
    return bool(lib().wpt_kernel_launch_record())


def material_places(node_count, tri_count, material_count, behind_corners, instance_count, hotspot_count):
    """wpt_material_places: (read by LDS address?, first quadword, quadwords of the scene) for a launch in the large form"""
    at, quads = C.c_uint32(0), C.c_uint32(0)
    fits = lib().wpt_material_places(node_count, tri_count, material_count, 1 if behind_corners else 0, instance_count, hotspot_count,
                                     C.byref(at), C.byref(quads))
    return bool(fits), at.value, quads.value


def fold_plan(host_scene, with_words=False):
    """wpt_fold_plan: the nodes whose link the kernels with the scene in LDS fold in their copy of the scene's tree; with
    with_words (count, word 7 of every node's LDS copy as numpy uint32).  Needs no device"""
    import numpy as np
    folded = C.c_uint32()
    words = np.zeros(int(host_scene.d.node_count), np.uint32)
    _check(lib().wpt_fold_plan(C.cast(host_scene.desc, C.c_void_p), C.byref(folded), _array_ptr(words if with_words else None)))
    return (int(folded.value), words) if with_words else int(folded.value)


BYPASS_MODEL, BYPASS_ALL_ELIGIBLE = 0, 1  # wpt_set_bypass


def set_bypass(mode):
    """wpt_set_bypass (tests): which eligible inner nodes the walk of a scene in LDS leaves out -- BYPASS_MODEL: the cost model's
    choice, BYPASS_ALL_ELIGIBLE: all of them; read when a scene is uploaded and by bypass_plan"""
    _check(lib().wpt_set_bypass(mode))


def bypass_plan(host_scene, with_words=False):
    """wpt_bypass_plan: the inner nodes that the walk of the scene's tree in LDS leaves out; with with_words (count, links, start):
    links[i] = (skip link, word 7) of node i's LDS copy as numpy uint32, start = the node a ray starts at.  Needs no device"""
    import numpy as np
    count = C.c_uint32()
    n = int(host_scene.d.node_count)
    words = np.zeros(2 * n + 1, np.uint32)
    _check(lib().wpt_bypass_plan(C.cast(host_scene.desc, C.c_void_p), C.byref(count), _array_ptr(words if with_words else None)))
    return (int(count.value), words[:2 * n].reshape(n, 2), int(words[2 * n])) if with_words else int(count.value)


def progress_covers(sensor=SENSOR_FRAME, counting=False, bands=False):
    """wpt_progress_covers: raises RuntimeError with the library's reason if progressive sessions do not cover such a launch;
    needs no device"""
    _check(lib().wpt_progress_covers(sensor, int(bool(counting)), int(bool(bands))))


def progress_state_info(state):
    """wpt_progress_state_info: the header of a saved session as a dict (version, width, height, samples_sqrt, block_start,
    block_size, rows_done, tag, state_bytes); a state that is not a good one is refused with RuntimeError.  Needs no device."""
    state = bytes(state)
    info = _abi.ProgressInfo()
    _check(lib().wpt_progress_state_info(state, len(state), C.byref(info)))
    return {n: int(getattr(info, n)) for n, _ in info._fields_ if n != "reserved"}


class Progressive:
    """A progressive session of a DeviceScene (wurblpt_hip.h, wpt_progress_*): the block's pixels of one frame rendered in
    stages of rows of strata.  The finished frame is bit for bit DeviceScene.render's; previews are pictures to look at."""

    def __init__(self, scene, handle, width, height, block):
        self.scene, self._handle = scene, handle
        self.width, self.height, self.block = width, height, block

    @property
    def rows_done(self):
        return int(lib().wpt_progress_rows_done(self._handle))

    @property
    def rows_total(self):
        return int(lib().wpt_progress_rows_total(self._handle))

    @property
    def finished(self):
        return self.rows_done == self.rows_total

    def advance(self, rows, frame=None, stream=None):
        """Renders up to `rows` further rows of strata, asynchronously on `stream` (None: the default stream).  `frame`: CUDA
        float32 tensor [h, w, 3] that the stage which finishes the session writes the block's pixels of; earlier stages do not
        touch it and need none.  Returns rows_done."""
        if frame is not None:
            assert frame.is_cuda and frame.is_contiguous() and frame.dtype.is_floating_point and frame.element_size() == 4
            assert frame.numel() == self.width * self.height * 3
        _check(lib().wpt_progress_advance_device(self._handle, rows, _tensor_ptr(frame), _stream_ptr(stream)))
        return self.rows_done

    def preview(self, out=None, stream=None):
        """The preview as a CUDA float32 tensor [h, w, 3] (zeros outside the block; `out`: written in place, and left as it is
        outside the block), asynchronously on `stream`."""
        import torch
        if out is None:
            out = torch.zeros((self.height, self.width, 3), dtype=torch.float32, device="cuda")
            if stream is not None:
                stream.wait_stream(torch.cuda.current_stream())
        assert out.is_cuda and out.is_contiguous() and out.element_size() == 4 and out.numel() == self.width * self.height * 3
        _check(lib().wpt_progress_preview_device(self._handle, C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
        return out

    def save(self):
        """wpt_progress_save: the session's state as bytes (waits for the session's last stream)"""
        n = C.c_uint64()
        _check(lib().wpt_progress_state_bytes(self._handle, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().wpt_progress_save(self._handle, buf, n.value))
        return buf.raw

    def close(self):
        if self._handle:
            lib().wpt_progress_end(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceScene:
    """A flattened scene resident in HBM on the current device."""

    def __init__(self, host_scene):
        self._handle = C.c_void_p()
        _check(lib().wpt_scene_upload(host_scene.desc, C.byref(self._handle)))
        self.host = host_scene

    def bypassed_nodes(self):
        """wpt_scene_bypassed_nodes: the inner nodes the walk leaves out, chosen at the upload"""
        count = C.c_uint32()
        _check(lib().wpt_scene_bypassed_nodes(self._handle, C.byref(count)))
        return int(count.value)

    def folded_links(self):
        """wpt_scene_folded_links: the folded nodes, counted at the upload"""
        folded = C.c_uint32()
        _check(lib().wpt_scene_folded_links(self._handle, C.byref(folded)))
        return int(folded.value)

    def close(self):
        """Frees the scene.  Progressive sessions of it must be closed first: they read the scene in every stage."""
        if self._handle:
            lib().wpt_scene_free(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self):
        """Synchronises and raises if a launch on this scene aborted."""
        _check(lib().wpt_scene_check(self._handle))

    def render_block_into(self, frame, samples_sqrt, block=None, params=None, counters=None, stream=None,
                          width=None, height=None):
        """Asynchronously renders pixels [start, start+size) into `frame`, a CUDA float32 tensor
        [h, w, 3] (full frame).  `counters`: optional CUDA int64 tensor [6] that is added to."""
        w, h = _frame_size(self.host, width, height)
        assert frame.is_cuda and frame.is_contiguous() and frame.numel() == w * h * 3
        p = _params(params)
        start, size = block if block is not None else (0, w * h)
        _check(lib().wpt_render_block_device(self._handle, self.host.camera, C.byref(p), w, h, samples_sqrt,
                                              start, size, C.c_void_p(frame.data_ptr()), _tensor_ptr(counters), _stream_ptr(stream)))

    def render_bands_into(self, frame, samples_sqrt, band_rows, first_band, band_stride, params=None, counters=None, stream=None,
                          width=None, height=None):
        """Asynchronously renders bands first_band, first_band + band_stride, ... of `band_rows` rows each into `frame`
        (one launch: a rank's interleaved share of the frame)."""
        w, h = _frame_size(self.host, width, height)
        assert frame.is_cuda and frame.is_contiguous() and frame.numel() == w * h * 3
        p = _params(params)
        _check(lib().wpt_render_bands_device(self._handle, C.cast(self.host.camera, C.c_void_p), C.addressof(p), w, h, samples_sqrt,
                                             band_rows, first_band, band_stride, C.c_void_p(frame.data_ptr()), _tensor_ptr(counters),
                                             _stream_ptr(stream)))

    def render(self, samples_sqrt, block=None, params=None, with_counters=False, width=None, height=None):
        """Synchronous convenience: returns (frame as numpy [h, w, 3], counters dict or None)."""
        import torch
        w, h = _frame_size(self.host, width, height)
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        counters = _new_counters(with_counters)
        stream = torch.cuda.current_stream()
        self.render_block_into(frame, samples_sqrt, block, params, counters, stream, w, h)
        torch.cuda.synchronize()
        self.check()
        return frame.cpu().numpy(), _counters_dict(counters) if with_counters else None

    def render_shutter_into(self, frame, samples_sqrt, shutter, block=None, params=None, counters=None, stream=None,
                            width=None, height=None):
        """render_block_into under a rolling shutter (host.shutter): row r of the frame, whatever the block, is exposed over
        shutter_row_interval(shutter, params.t0, params.t1, h, r) and is bit for bit that row of the plain render with it."""
        w, h = _frame_size(self.host, width, height)
        assert frame.is_cuda and frame.is_contiguous() and frame.numel() == w * h * 3
        p = _params(params)
        start, size = block if block is not None else (0, w * h)
        _check(lib().wpt_render_shutter_block_device(self._handle, self.host.camera, C.byref(p), C.byref(shutter), w, h, samples_sqrt,
                                                      start, size, C.c_void_p(frame.data_ptr()), _tensor_ptr(counters), _stream_ptr(stream)))

    def render_shutter_bands_into(self, frame, samples_sqrt, shutter, band_rows, first_band, band_stride, params=None, counters=None,
                                  stream=None, width=None, height=None):
        """render_bands_into under a rolling shutter; the rows keep the intervals they have in the frame."""
        w, h = _frame_size(self.host, width, height)
        assert frame.is_cuda and frame.is_contiguous() and frame.numel() == w * h * 3
        p = _params(params)
        _check(lib().wpt_render_shutter_bands_device(self._handle, self.host.camera, C.byref(p), C.byref(shutter), w, h, samples_sqrt,
                                                     band_rows, first_band, band_stride, C.c_void_p(frame.data_ptr()), _tensor_ptr(counters),
                                                     _stream_ptr(stream)))

    def render_shutter(self, samples_sqrt, shutter, block=None, params=None, with_counters=False, width=None, height=None):
        """Synchronous convenience, as render: (frame as numpy [h, w, 3], counters dict or None)."""
        import torch
        w, h = _frame_size(self.host, width, height)
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        counters = _new_counters(with_counters)
        self.render_shutter_into(frame, samples_sqrt, shutter, block, params, counters, torch.cuda.current_stream(), w, h)
        torch.cuda.synchronize()
        self.check()
        return frame.cpu().numpy(), _counters_dict(counters) if with_counters else None

    def render_shutter_host(self, samples_sqrt, shutter, block=None, bands=None, params=None, width=None, height=None):
        """The synchronous forms for host memory.  block = (start, size): wpt_render_shutter_block, the block's pixels as
        [size, 3]; bands = (band_rows, first_band, band_stride): wpt_render_shutter_bands, the full frame [h, w, 3] with the
        other bands left at zero."""
        import numpy as np
        w, h = _frame_size(self.host, width, height)
        p = _params(params)
        if (block is None) == (bands is None):
            raise ValueError("render_shutter_host: give block or bands")
        if block is not None:
            start, size = block
            out = np.zeros((size, 3), dtype=np.float32)
            _check(lib().wpt_render_shutter_block(self._handle, self.host.camera, C.byref(p), C.byref(shutter), w, h, samples_sqrt, start, size,
                                                   C.c_void_p(out.ctypes.data)))
            return out
        band_rows, first_band, band_stride = bands
        out = np.zeros((h, w, 3), dtype=np.float32)
        _check(lib().wpt_render_shutter_bands(self._handle, self.host.camera, C.byref(p), C.byref(shutter), w, h, samples_sqrt, band_rows,
                                               first_band, band_stride, C.c_void_p(out.ctypes.data)))
        return out

    def progressive(self, samples_sqrt, block=None, params=None, width=None, height=None, tag=None, sensor=SENSOR_FRAME,
                    with_counters=False, bands=False):
        """wpt_progress_begin: a Progressive session for `block` (default: the whole frame).  `tag`: the caller's fingerprint of
        the scene, kept in saved states (default: host.scene_tag of this scene).  sensor, with_counters, bands: what kind of
        launch the session is to stand for; anything but one plain frame is refused with the library's reason."""
        from . import host
        progress_covers(sensor, with_counters, bands)
        w, h = _frame_size(self.host, width, height)
        p = _params(params)
        start, size = block if block is not None else (0, w * h)
        handle = C.c_void_p()
        _check(lib().wpt_progress_begin(self._handle, self.host.camera, C.byref(p), w, h, samples_sqrt, start, size,
                                        host.scene_tag(self.host) if tag is None else tag, C.byref(handle)))
        return Progressive(self, handle, w, h, (start, size))

    def resume(self, state, params=None, tag=None, samples_sqrt=None):
        """wpt_progress_restore: the session a Progressive.save() was taken from, for this scene's camera.  The state's tag,
        camera and params must be the ones given here (RuntimeError names the first that differs); `samples_sqrt`, if given, is
        compared with the state's as well."""
        from . import host
        state = bytes(state)
        info = progress_state_info(state)
        if samples_sqrt is not None and int(samples_sqrt) != info["samples_sqrt"]:
            raise RuntimeError("wurblpt_hip: the state was saved with a different samples_sqrt (%d, not %d)" % (info["samples_sqrt"], samples_sqrt))
        p = _params(params)
        handle = C.c_void_p()
        _check(lib().wpt_progress_restore(self._handle, state, len(state), self.host.camera, C.byref(p),
                                          host.scene_tag(self.host) if tag is None else tag, C.byref(handle)))
        return Progressive(self, handle, info["width"], info["height"], (info["block_start"], info["block_size"]))

    def render_stages(self, samples_sqrt, rows_per_stage=None, seconds_per_stage=None, block=None, params=None, width=None, height=None,
                      tag=None):
        """Generator over the stages of one frame: yields (rows_done, preview) after every stage that does not finish the frame
        and (samples_sqrt, frame) at the end, both CUDA tensors [h, w, 3]; the frame is DeviceScene.render's bit for bit.
        rows_per_stage: rows of strata per stage (default 1).  seconds_per_stage: the first stage renders one row, and every
        further one as many rows as fit that time by the measured time per row of the stage before, at least 1."""
        import time
        import torch
        session = self.progressive(samples_sqrt, block, params, width, height, tag)
        try:
            frame = torch.zeros((session.height, session.width, 3), dtype=torch.float32, device="cuda")
            stream = torch.cuda.current_stream()
            rows = 1 if seconds_per_stage is not None else max(1, int(rows_per_stage or 1))
            while not session.finished:
                before = session.rows_done
                torch.cuda.synchronize()
                start = time.perf_counter()
                session.advance(rows, frame, stream)
                torch.cuda.synchronize()
                self.check()
                per_row = (time.perf_counter() - start) / (session.rows_done - before)
                if seconds_per_stage is not None:
                    rows = max(1, int(min(float(samples_sqrt), seconds_per_stage / per_row))) if per_row > 0 else samples_sqrt
                if not session.finished:
                    yield session.rows_done, session.preview(stream=stream)
            yield session.rows_done, frame
        finally:
            session.close()

    def render_transient_into(self, frame, bins, samples_sqrt, edges, block=None, params=None, stream=None, width=None, height=None):
        """Asynchronously renders pixels [start, start+size) of the frame and of the transient film in one launch.
        `frame`: CUDA float32 tensor [h, w, 3] or None; `bins`: CUDA float32 tensor [K, h, w, 3] (full frames);
        `edges`: K + 1 increasing floats (the last may be inf).  Bin k is the light whose optical path length lies in
        [edges[k], edges[k + 1]), per channel, behind the distance gate of `params`."""
        w, h = _frame_size(self.host, width, height)
        e = _edges_array(edges)
        K = e.size - 1
        assert bins.is_cuda and bins.is_contiguous() and bins.dtype.is_floating_point and bins.element_size() == 4 and bins.numel() == K * w * h * 3
        if frame is not None:
            assert frame.is_cuda and frame.is_contiguous() and frame.numel() == w * h * 3
        p = _params(params)
        start, size = block if block is not None else (0, w * h)
        _check(lib().wpt_render_transient_block_device(self._handle, self.host.camera, C.byref(p), C.c_void_p(e.ctypes.data), K,
                                                        w, h, samples_sqrt, start, size, _tensor_ptr(frame), C.c_void_p(bins.data_ptr()),
                                                        _stream_ptr(stream)))

    def render_transient(self, samples_sqrt, edges, block=None, params=None, width=None, height=None):
        """Synchronous convenience: returns (frame [h, w, 3], bins [K, h, w, 3]) as numpy arrays."""
        import torch
        w, h = _frame_size(self.host, width, height)
        K = _edges_array(edges).size - 1
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        bins = torch.zeros((K, h, w, 3), dtype=torch.float32, device="cuda")
        self.render_transient_into(frame, bins, samples_sqrt, edges, block, params, torch.cuda.current_stream(), w, h)
        torch.cuda.synchronize()
        self.check()
        return frame.cpu().numpy(), bins.cpu().numpy()

    def render_transient_host(self, samples_sqrt, edges, block, params=None, width=None, height=None):
        """wpt_render_transient_block: submitBlock semantics; returns (block rgb [size, 3], block bins [K, size, 3])."""
        import numpy as np
        w, h = _frame_size(self.host, width, height)
        e = _edges_array(edges)
        K = e.size - 1
        p = _params(params)
        start, size = block
        rgb = np.zeros((size, 3), dtype=np.float32)
        bins = np.zeros((K, size, 3), dtype=np.float32)
        _check(lib().wpt_render_transient_block(self._handle, self.host.camera, C.byref(p), C.c_void_p(e.ctypes.data), K, w, h,
                                                samples_sqrt, start, size, C.c_void_p(rgb.ctypes.data), C.c_void_p(bins.ctypes.data)))
        return rgb, bins

    def render_light_groups_into(self, frame, planes, samples_sqrt, groups, group_count, env_group=_abi.LIGHT_GROUP_NONE, block=None,
                                 params=None, stream=None, width=None, height=None):
        """Asynchronously renders pixels [start, start+size) of the frame and of a plane per group of emitters in one launch.
        `frame`: CUDA float32 tensor [h, w, 3] or None; `planes`: CUDA float32 tensor [K, h, w, 3] (full frames), K = group_count;
        `groups`: one integer per material record of the scene (host.emitters lists those that emit), a group below K or
        _abi.LIGHT_GROUP_NONE; `env_group`: the environment's.  Plane g is bit for bit the plain render of the scene in which
        only group g emits (host.mute_emitters); both gates of `params` apply to the planes as to the frame."""
        w, h = _frame_size(self.host, width, height)
        t = _groups_table(groups, self.host.d.material_count)
        K = int(group_count)
        assert planes.is_cuda and planes.is_contiguous() and planes.dtype.is_floating_point and planes.element_size() == 4 \
            and planes.numel() == K * w * h * 3
        if frame is not None:
            assert frame.is_cuda and frame.is_contiguous() and frame.numel() == w * h * 3
        p = _params(params)
        start, size = block if block is not None else (0, w * h)
        _check(lib().wpt_render_light_groups_block_device(self._handle, self.host.camera, C.byref(p), C.c_void_p(t.ctypes.data), t.size, K,
                                                           int(env_group), w, h, samples_sqrt, start, size, _tensor_ptr(frame),
                                                           C.c_void_p(planes.data_ptr()), _stream_ptr(stream)))

    def render_light_groups(self, samples_sqrt, groups, group_count, env_group=_abi.LIGHT_GROUP_NONE, block=None, params=None,
                            width=None, height=None):
        """Synchronous convenience: returns (frame [h, w, 3], planes [K, h, w, 3]) as numpy arrays."""
        import torch
        w, h = _frame_size(self.host, width, height)
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        planes = torch.zeros((int(group_count), h, w, 3), dtype=torch.float32, device="cuda")
        self.render_light_groups_into(frame, planes, samples_sqrt, groups, group_count, env_group, block, params,
                                      torch.cuda.current_stream(), w, h)
        torch.cuda.synchronize()
        self.check()
        return frame.cpu().numpy(), planes.cpu().numpy()

    def render_light_groups_host(self, samples_sqrt, groups, group_count, block, env_group=_abi.LIGHT_GROUP_NONE, params=None,
                                 width=None, height=None):
        """wpt_render_light_groups_block: submitBlock semantics; returns (block rgb [size, 3], block planes [K, size, 3])."""
        import numpy as np
        w, h = _frame_size(self.host, width, height)
        t = _groups_table(groups, self.host.d.material_count)
        K = int(group_count)
        p = _params(params)
        start, size = block
        rgb = np.zeros((size, 3), dtype=np.float32)
        planes = np.zeros((K, size, 3), dtype=np.float32)
        _check(lib().wpt_render_light_groups_block(self._handle, self.host.camera, C.byref(p), C.c_void_p(t.ctypes.data), t.size, K,
                                                    int(env_group), w, h, samples_sqrt, start, size, C.c_void_p(rgb.ctypes.data),
                                                    C.c_void_p(planes.ctypes.data)))
        return rgb, planes

    def render_tof_into(self, planes, samples_sqrt, sensor, phases=None, block=None, params=None, stream=None):
        """Asynchronously renders pixels [start, start+size) of the time-of-flight sensor's phase images in one launch.
        `planes`: CUDA float32 tensor [n, h, w, 3] = (a, b, total) per phase image; `sensor`: host.tof_sensor(...);
        `phases`: indices of the sensor's phase images to render (default: all of them, n = sensor.phase_count).  Plane j is
        bit for bit the one-phase launch of that phase; `params` must carry the default gates."""
        w, h = self.host.width, self.host.height
        s = _tof_phases(sensor, phases)
        assert planes.is_cuda and planes.is_contiguous() and planes.dtype.is_floating_point and planes.element_size() == 4 \
            and planes.numel() == s.phase_count * w * h * 3
        p = _params(params)
        start, size = block if block is not None else (0, w * h)
        _check(lib().wpt_render_tof_block_device(self._handle, self.host.camera, C.byref(p), C.byref(s), w, h, samples_sqrt, start, size,
                                                  C.c_void_p(planes.data_ptr()), _stream_ptr(stream)))

    def render_tof(self, samples_sqrt, sensor, phases=None, block=None, params=None):
        """Synchronous convenience: returns the planes [n, h, w, 3] as a numpy array (pixels outside `block` are 0)."""
        import torch
        w, h = self.host.width, self.host.height
        n = _tof_phases(sensor, phases).phase_count
        planes = torch.zeros((n, h, w, 3), dtype=torch.float32, device="cuda")
        self.render_tof_into(planes, samples_sqrt, sensor, phases, block, params, torch.cuda.current_stream())
        torch.cuda.synchronize()
        self.check()
        return planes.cpu().numpy()

    def render_tof_host(self, samples_sqrt, sensor, block, phases=None, params=None):
        """wpt_render_tof_block: submitBlock semantics; returns the block's planes [n, size, 3]."""
        import numpy as np
        w, h = self.host.width, self.host.height
        s = _tof_phases(sensor, phases)
        p = _params(params)
        start, size = block
        planes = np.zeros((s.phase_count, size, 3), dtype=np.float32)
        _check(lib().wpt_render_tof_block(self._handle, self.host.camera, C.byref(p), C.byref(s), w, h, samples_sqrt, start, size,
                                           C.c_void_p(planes.ctypes.data)))
        return planes

    def _views_args(self, frames, cameras, params):
        """(camera array, V, params, w, h) of a launch of a batch of views into `frames`, checked to be [V, h, w, 3]"""
        V = len(cameras)
        assert frames.is_cuda and frames.is_contiguous() and frames.dtype.is_floating_point and frames.element_size() == 4
        assert frames.dim() == 4 and frames.shape[0] == V and frames.shape[3] == 3, "frames: [V, h, w, 3]"
        return (_abi.Camera * max(V, 1))(*cameras), V, _params(params), int(frames.shape[2]), int(frames.shape[1])

    def render_views_into(self, frames, cameras, samples_sqrt, params=None, counters=None, stream=None):
        """Asynchronously renders a batch of views in one launch: frame v of `frames`, a CUDA float32 tensor [V, h, w, 3], from
        cameras[v] (_abi.Camera records, e.g. host.camera_looking_at).  One parameter set, frame size and sample count serve all
        views; frame v is bit for bit the plain render of cameras[v].  `counters`: optional CUDA int64 tensor [6] that the sum
        over all views is added to."""
        cams, V, p, w, h = self._views_args(frames, cameras, params)
        _check(lib().wpt_render_views_device(self._handle, cams, V, C.byref(p), w, h, samples_sqrt, C.c_void_p(frames.data_ptr()),
                                             _tensor_ptr(counters), _stream_ptr(stream)))

    def render_view_streams_into(self, frames, cameras, samples_sqrt, streams=None, params=None, counters=None, stream=None):
        """render_views_into with a sample stream per view: view v is stream streams[v] of cameras[v], i.e. pixel p's generator is
        seeded from p + streams[v] * w * h (in 64 bits) instead of p.  `streams`: V integers in [0, 2^32), or None for all 0,
        which is render_views_into.  Stream 0 is the plain render bit for bit."""
        import numpy as np
        cams, V, p, w, h = self._views_args(frames, cameras, params)
        ks = None
        if streams is not None:
            if len(streams) != V or any(not 0 <= int(k) < 2 ** 32 for k in streams):
                raise ValueError("streams: one integer in [0, 2^32) per view")
            ks = np.ascontiguousarray(np.array([int(k) for k in streams], dtype=np.uint32))
        _check(lib().wpt_render_view_streams_device(self._handle, cams, _array_ptr(ks if V else None), V, C.byref(p), w, h, samples_sqrt,
                                                    C.c_void_p(frames.data_ptr()), _tensor_ptr(counters), _stream_ptr(stream)))

    def _render_views(self, into, cameras, with_counters, width, height):
        """the synchronous form of a batch of views, launched by into(frames, counters, stream)"""
        import torch
        w, h = _frame_size(self.host, width, height)
        frames = torch.zeros((len(cameras), h, w, 3), dtype=torch.float32, device="cuda")
        counters = _new_counters(with_counters)
        into(frames, counters, torch.cuda.current_stream())
        torch.cuda.synchronize()
        self.check()
        return (frames, _counters_dict(counters)) if with_counters else frames

    def render_views(self, samples_sqrt, cameras, params=None, with_counters=False, width=None, height=None):
        """Synchronous convenience: returns the frames as a CUDA tensor [V, h, w, 3] (and the counters dict with_counters)."""
        return self._render_views(lambda frames, counters, stream: self.render_views_into(frames, cameras, samples_sqrt, params, counters, stream),
                                  cameras, with_counters, width, height)

    def render_view_streams(self, samples_sqrt, cameras, streams=None, params=None, with_counters=False, width=None, height=None):
        """Synchronous convenience: returns the frames as a CUDA tensor [V, h, w, 3] (and the counters dict with_counters)."""
        return self._render_views(lambda frames, counters, stream: self.render_view_streams_into(frames, cameras, samples_sqrt, streams, params,
                                                                                                 counters, stream),
                                  cameras, with_counters, width, height)

    def render_split_into(self, frame, stream_samples_sqrt, streams, first=0, moments=None, params=None, counters=None, stream=None,
                          camera=None):
        """wpt_render_split_device: the scene's camera (or `camera`) rendered in `streams` sample streams first .. first + streams - 1
        of stream_samples_sqrt^2 samples each, in one launch of the batch-of-views kernels, and reduced to their mean in `frame`,
        a CUDA float32 tensor [h, w, 3]; `moments` (optional, the same shape): the stream moment film, the mean of the stream
        frames' squares.  Asynchronous on `stream`; the scratch (streams * h * w * 12 bytes) is allocated and freed in stream
        order.  `counters`: optional CUDA int64 tensor [6] that the sum over all streams is added to."""
        assert frame.is_cuda and frame.is_contiguous() and frame.dtype.is_floating_point and frame.element_size() == 4
        assert frame.dim() == 3 and frame.shape[2] == 3, "frame: [h, w, 3]"
        h, w = int(frame.shape[0]), int(frame.shape[1])
        if moments is not None:
            assert moments.is_cuda and moments.is_contiguous() and moments.dtype.is_floating_point and moments.element_size() == 4
            assert tuple(moments.shape) == tuple(frame.shape), "moments: the frame's shape"
        if not (0 <= int(streams) < 2 ** 32 and 0 <= int(first) < 2 ** 32):
            raise ValueError("render_split: streams and first are 32-bit counts")
        p = _params(params)
        cam = C.byref(camera) if camera is not None else self.host.camera
        _check(lib().wpt_render_split_device(self._handle, cam, C.byref(p), w, h, stream_samples_sqrt, int(first), int(streams),
                                             C.c_void_p(frame.data_ptr()), _tensor_ptr(moments), _tensor_ptr(counters), _stream_ptr(stream)))

    def render_split(self, stream_samples_sqrt, streams, first=0, with_moments=False, params=None, with_counters=False, width=None,
                     height=None, camera=None):
        """Synchronous convenience: returns the frame as numpy [h, w, 3]; with_moments (frame, moments); with_counters the counters
        dict as a last element as well."""
        import torch
        w, h = _frame_size(self.host, width, height)
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        moments = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") if with_moments else None
        counters = _new_counters(with_counters)
        self.render_split_into(frame, stream_samples_sqrt, streams, first, moments, params, counters, torch.cuda.current_stream(), camera)
        torch.cuda.synchronize()
        self.check()
        out = [frame.cpu().numpy()]
        if with_moments:
            out.append(moments.cpu().numpy())
        if with_counters:
            out.append(_counters_dict(counters))
        return out[0] if len(out) == 1 else tuple(out)

    def render_adaptive_into(self, frame, samples_sqrt, moments=None, block=None, params=None, stream=None):
        """Renders pixels [start, start+size) with a sample-count map on `stream` (None: torch's current stream): pixel p with
        n_p^2 samples, bit for bit the plain render at samples_sqrt = n_p; pixels with n_p = 0 are not rendered and their
        entries not written.  `samples_sqrt`: integer map [h, w] with values in [0, 65535] (any integer tensor or array);
        `frame` and `moments` (optional: the moment film, 1 / n_p^2 times the sum of the squares of what each sample added):
        CUDA float32 [h, w, 3].  The launch is ordered behind the work on torch's current stream, so inputs made there are
        ready.  Asynchronous for a CUDA map of torch.uint16; a CUDA map of another integer type is range-checked on the
        device, which reads one flag back (a sync of the current stream); a host map is checked on the host and uploaded."""
        import torch
        if not (isinstance(samples_sqrt, torch.Tensor) and samples_sqrt.is_cuda):
            _map_int(samples_sqrt)
        assert len(samples_sqrt.shape) == 2, "samples_sqrt: [h, w]"
        h, w = int(samples_sqrt.shape[0]), int(samples_sqrt.shape[1])
        assert frame.is_cuda and frame.is_contiguous() and frame.dtype.is_floating_point and frame.element_size() == 4 and frame.numel() == w * h * 3
        if moments is not None:
            assert moments.is_cuda and moments.is_contiguous() and moments.dtype.is_floating_point and moments.element_size() == 4
            assert moments.numel() == w * h * 3
        current = torch.cuda.current_stream()
        launch = stream if stream is not None else current
        # the 16-bit map is made on the current stream (where the caller's map was written); the launch stream waits for it
        m16 = _map_u16_device(samples_sqrt)
        if launch != current:
            launch.wait_stream(current)
            m16.record_stream(launch)                   # freed only after the launch stream's use
        p = _params(params)
        start, size = block if block is not None else (0, w * h)
        _check(lib().wpt_render_adaptive_block_device(self._handle, self.host.camera, C.byref(p), w, h, C.c_void_p(m16.data_ptr()),
                                                       start, size, C.c_void_p(frame.data_ptr()), _tensor_ptr(moments), _stream_ptr(launch)))

    def render_adaptive(self, samples_sqrt, with_moments=False, block=None, params=None):
        """Synchronous convenience: returns the frame as a new CUDA tensor [h, w, 3] (zeros where n_p = 0), and with_moments
        the moment film as well: (frame, moments)."""
        import torch
        h, w = int(samples_sqrt.shape[0]), int(samples_sqrt.shape[1])
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        moments = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") if with_moments else None
        self.render_adaptive_into(frame, samples_sqrt, moments, block, params, torch.cuda.current_stream())
        torch.cuda.synchronize()
        self.check()
        return (frame, moments) if with_moments else frame

    def render_adaptive_host(self, samples_sqrt, block, block_rgb, block_moments=None, params=None):
        """wpt_render_adaptive_block: submitBlock semantics.  `block_rgb` and `block_moments` (or None): numpy float32
        [size, 3], written in place for the block's pixels with n_p > 0 and left as they are elsewhere."""
        import numpy as np
        a = _map_int(samples_sqrt)
        h, w = a.shape
        m = np.ascontiguousarray(a.astype(np.uint16))
        p = _params(params)
        start, size = block
        for b in (block_rgb, block_moments):
            assert b is None or (b.dtype == np.float32 and b.flags.c_contiguous and b.size == size * 3)
        _check(lib().wpt_render_adaptive_block(self._handle, self.host.camera, C.byref(p), w, h, C.c_void_p(m.ctypes.data), start, size,
                                               C.c_void_p(block_rgb.ctypes.data), _array_ptr(block_moments)))
        return block_rgb, block_moments

    def render_block_host(self, samples_sqrt, block, params=None, width=None, height=None):
        """wpt_render_block: MPICoordinator::submitBlock semantics, host buffer of size*3 floats."""
        import numpy as np
        w, h = _frame_size(self.host, width, height)
        p = _params(params)
        start, size = block
        out = np.zeros((size, 3), dtype=np.float32)
        _check(lib().wpt_render_block(self._handle, self.host.camera, C.byref(p), w, h, samples_sqrt, start, size,
                                       C.c_void_p(out.ctypes.data)))
        return out

    def ground_truth_device(self, bits=None, camera_prev=None, camera_next=None, params=None, width=None, height=None, times=None,
                            stream=None):
        """wpt_ground_truth_device: dict name -> CUDA tensor [h, w, comps] (float32; "materials": int32) of the requested
        GroundTruth bits (None: the three arrays a denoiser call reads, GUIDE_NAMES), left in device memory.  Asynchronous on
        `stream` (None: torch's current stream).  times = (t0, tPrev, tNext) for animated instances."""
        import torch
        if bits is None:
            bits = sum(1 << GT_NAMES.index(name) for name in GUIDE_NAMES)
        w, h = _frame_size(self.host, width, height)
        p = _params(params)
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            arrays = _gt_alloc(torch, w, h, bits, device="cuda")
        ptrs = (C.c_void_p * 20)(*[a.data_ptr() if a is not None else None for a in arrays])
        tm = (C.c_float * 3)(*times) if times is not None else None
        _check(lib().wpt_ground_truth_device(self._handle, C.cast(self.host.camera, C.c_void_p),
                                             C.addressof(camera_prev) if camera_prev is not None else None,
                                             C.addressof(camera_next) if camera_next is not None else None, tm, C.addressof(p), w, h, ptrs,
                                             C.c_void_p(s.cuda_stream)))
        return {GT_NAMES[k]: a for k, a in enumerate(arrays) if a is not None}

    def first_hit_colours_device(self, albedo=True, emission=True, guide=True, params=None, width=None, height=None, stream=None):
        """wpt_first_hit_colours_device: dict of CUDA tensors left in device memory: "albedo" and "emission" (float32 [h, w, 3]) and,
        with `guide`, the three arrays of GUIDE_NAMES as ground_truth_device returns them, from the same walk: the dict can be
        handed to denoise / denoise_demodulated as the guide.  The picture is taken at params.t0.  Asynchronous on `stream`
        (None: torch's current stream)."""
        import torch
        w, h = _frame_size(self.host, width, height)
        p = _params(params)
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            out = _first_hit_alloc(torch, w, h, albedo, emission, guide, device="cuda")
        ptrs = (C.c_void_p * 3)(*[out[name].data_ptr() for name in GUIDE_NAMES]) if guide else None
        _check(lib().wpt_first_hit_colours_device(self._handle, C.cast(self.host.camera, C.c_void_p), C.addressof(p), w, h,
                                                  _tensor_ptr(out.get("albedo")), _tensor_ptr(out.get("emission")), ptrs, C.c_void_p(s.cuda_stream)))
        return out


def first_hit_colours(scene, albedo=True, emission=True, guide=True, params=None, width=None, height=None):
    """wpt_first_hit_colours on a DeviceScene: the dict of DeviceScene.first_hit_colours_device as numpy arrays (synchronous)"""
    import numpy as np
    w, h = _frame_size(scene.host, width, height)
    p = _params(params)
    out = _first_hit_alloc(np, w, h, albedo, emission, guide)
    ptrs = (C.c_void_p * 3)(*[out[name].ctypes.data for name in GUIDE_NAMES]) if guide else None
    _check(lib().wpt_first_hit_colours(scene._handle, C.cast(scene.host.camera, C.c_void_p), C.addressof(p), w, h,
                                       _array_ptr(out.get("albedo")), _array_ptr(out.get("emission")), ptrs))
    return out


GT_NAMES = ("world_space_positions", "world_space_geometry_normals", "world_space_geometry_tangents",
            "world_space_material_normals", "world_space_material_tangents", "camera_space_positions",
            "camera_space_geometry_normals", "camera_space_geometry_tangents", "camera_space_material_normals",
            "camera_space_material_tangents", "camera_space_depths", "camera_space_distances", "texcoords",
            "world_space_offset_to_prev", "world_space_offset_to_next", "camera_space_offset_to_prev",
            "camera_space_offset_to_next", "pixel_space_offset_to_prev", "pixel_space_offset_to_next", "materials")
GT_COMPONENTS = (3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 1, 1, 2, 3, 3, 3, 3, 2, 2, 1)
GT_ALL = (1 << 20) - 1


def _gt_alloc(xp, width, height, bits, **where):
    """The zeroed outputs of a ground truth call from the array maker `xp` (numpy, or torch with where = its device): a list of
    20, array k [height, width, GT_COMPONENTS[k]] (float32; "materials": int32) where bit k of `bits` is set and None elsewhere"""
    return [xp.zeros((height, width, GT_COMPONENTS[k]), dtype=xp.int32 if GT_NAMES[k] == "materials" else xp.float32, **where)
            if bits & (1 << k) else None for k in range(20)]


def _first_hit_alloc(xp, width, height, albedo, emission, guide, **where):
    """the zeroed outputs of a first-hit call as a dict: "albedo" and "emission" where wanted and, with `guide`, GUIDE_NAMES"""
    out = {name: xp.zeros((height, width, 3), dtype=xp.float32, **where) for name, wanted in (("albedo", albedo), ("emission", emission)) if wanted}
    if guide:
        arrays = _gt_alloc(xp, width, height, sum(1 << GT_NAMES.index(name) for name in GUIDE_NAMES), **where)
        out.update((name, arrays[GT_NAMES.index(name)]) for name in GUIDE_NAMES)
    return out


def gt_arrays(width, height, bits=GT_ALL):
    """Host arrays for a ground truth call: (list of numpy arrays or None, ctypes pointer array)."""
    import numpy as np
    arrays = _gt_alloc(np, width, height, bits)
    ptrs = (C.c_void_p * 20)(*[a.ctypes.data if a is not None else None for a in arrays])
    return arrays, ptrs


def ground_truth(scene, bits=GT_ALL, camera_prev=None, camera_next=None, params=None, width=None, height=None, times=None):
    """wpt_ground_truth on a DeviceScene: dict name -> numpy array [h, w, comps] of the requested GroundTruth bits.
    times = (t0, tPrev, tNext) for animated instances."""
    w, h = _frame_size(scene.host, width, height)
    p = _params(params)
    arrays, ptrs = gt_arrays(w, h, bits)
    tm = (C.c_float * 3)(*times) if times is not None else None
    _check(lib().wpt_ground_truth(scene._handle, C.cast(scene.host.camera, C.c_void_p),
                                  C.addressof(camera_prev) if camera_prev is not None else None,
                                  C.addressof(camera_next) if camera_next is not None else None, tm, C.addressof(p), w, h, ptrs))
    return {GT_NAMES[k]: a for k, a in enumerate(arrays) if a is not None}


def postproc(op, rgb, a=0.0, b=0.0):
    """Output-side operations on a frame (float32 [..., 3]) through wpt_postproc_host: op "srgb" -> uint8 frame,
    "urq" (a = max_val, b = brightness) and "scale" (a = factor, b = clamp) -> float frames, "maxlum" -> float."""
    import numpy as np
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    pixels = rgb.size // 3
    code = {"srgb": 0, "urq": 1, "scale": 2, "maxlum": 3}[op]
    out = np.zeros(rgb.shape, np.uint8) if code == 0 else (np.zeros(1, np.float32) if code == 3 else np.zeros(rgb.shape, np.float32))
    _check(lib().wpt_postproc_host(code, C.c_void_p(rgb.ctypes.data), C.c_void_p(out.ctypes.data), pixels, a, b))
    return float(out[0]) if code == 3 else out


def selftest_aabb(boxes, rays):
    """AABB::mayHit as the kernels evaluate it: boxes (n,6) lo hi, rays (n,8) origin dir amin amax."""
    import numpy as np
    import torch
    tb = torch.as_tensor(np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6), device="cuda")
    tr = torch.as_tensor(np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8), device="cuda")
    assert tb.shape[0] == tr.shape[0]
    out = torch.empty(tb.shape[0], dtype=torch.int32, device="cuda")
    _check(lib().wpt_selftest_aabb(tb.shape[0], C.c_void_p(tb.data_ptr()), C.c_void_p(tr.data_ptr()), C.c_void_p(out.data_ptr())))
    return out.cpu().numpy()


def selftest_triangle(form, cases):
    """The watertight triangle test as the kernels call it (wpt_selftest_triangle_kernel).  cases (n, 17): v0 v1 v2 origin
    direction amin amax; form 0 rayAux + triangleTest, 1 rayAuxRotated + triangleTestRotated, 2 and 3 their forms in the
    light-pdf loop, 4 form 1 through triangleTestRotatedStraight (the LDS kernels' leaf pass).  Returns uint32 (n, 8): accepted,
    the bits of a, invDet, U, V, W (zero when rejected), RayAux::k, spare."""
    import numpy as np
    import torch
    tc = torch.as_tensor(np.ascontiguousarray(cases, dtype=np.float32).reshape(-1, 17), device="cuda")
    out = torch.zeros((tc.shape[0], 8), dtype=torch.int32, device="cuda")
    _check(lib().wpt_selftest_triangle(form, tc.shape[0], C.c_void_p(tc.data_ptr()), C.c_void_p(out.data_ptr())))
    return out.cpu().numpy().view(np.uint32)


def selftest_rayaux(dirs):
    """The ray's constants as the kernels make them.  dirs (n, 3); returns float32 (n, 2, 9): inv (3), kx ky kz, S (3) from
    rayAux and from rayAuxRotated (its swap applied)."""
    import numpy as np
    import torch
    td = torch.as_tensor(np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3), device="cuda")
    out = torch.zeros((td.shape[0], 2, 9), dtype=torch.float32, device="cuda")
    _check(lib().wpt_selftest_rayaux(td.shape[0], C.c_void_p(td.data_ptr()), C.c_void_p(out.data_ptr())))
    return out.cpu().numpy()


def selftest_sphere(spheres, rays):
    """sphereTest as the kernels evaluate it: spheres (n, 4) centre radius, rays (n, 8) origin dir amin amax; returns float32
    (n, 2): accepted, a."""
    import numpy as np
    import torch
    ts = torch.as_tensor(np.ascontiguousarray(spheres, dtype=np.float32).reshape(-1, 4), device="cuda")
    tr = torch.as_tensor(np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8), device="cuda")
    assert ts.shape[0] == tr.shape[0]
    out = torch.zeros((ts.shape[0], 2), dtype=torch.float32, device="cuda")
    _check(lib().wpt_selftest_sphere(ts.shape[0], C.c_void_p(ts.data_ptr()), C.c_void_p(tr.data_ptr()), C.c_void_p(out.data_ptr())))
    return out.cpu().numpy()


def selftest_hits(scene, rays8):
    """The closest hit of a DeviceScene and its finished record for rays (n, 8) origin dir amin amax, at time 0: float32 (n, 15)
    in the layout of the restatement's bvh_hits (haveHit, prim, a, position, normal, tangent, texcoords, backside)."""
    import numpy as np
    import torch
    tr = torch.as_tensor(np.ascontiguousarray(rays8, dtype=np.float32).reshape(-1, 8), device="cuda")
    out = torch.zeros((tr.shape[0], 15), dtype=torch.float32, device="cuda")
    _check(lib().wpt_selftest_hits(scene._handle, tr.shape[0], C.c_void_p(tr.data_ptr()), C.c_void_p(out.data_ptr())))
    return out.cpu().numpy()


def selftest_math(op, a, b=None):
    """Evaluates one arithmetic primitive of the kernel on the GPU (see wpt_selftest_kernel)."""
    import torch
    ta = torch.as_tensor(a, dtype=torch.float32, device="cuda").contiguous()
    tb = torch.as_tensor(b if b is not None else a, dtype=torch.float32, device="cuda").contiguous()
    out = torch.empty_like(ta)
    _check(lib().wpt_selftest_math(op, ta.numel(), C.c_void_p(ta.data_ptr()), C.c_void_p(tb.data_ptr()), C.c_void_p(out.data_ptr())))
    return out.cpu().numpy()
