"""The marshalling of a frame stack into stk_frames (api._Marshalled), without a GPU: row-strided views — windows of a wider
image, rows padded — keep their own memory and hand their row step over as row_stride_bytes; every other layout is made
contiguous as before; and a contiguous stack produces the very stk_frames it always did (stride 0, the caller's pointers)."""
import ctypes as C

import numpy as np
import pytest

from libstacker_rs_amd import api
from libstacker_rs_amd.api import HOST, InvalidParams, _Marshalled

N, HC, WC = 4, 20, 31
Y0, X0, H, W = 3, 5, 11, 16


def _canvas(dtype=np.uint8, c=3):
    rng = np.random.default_rng(1)
    return rng.integers(0, 250, (N, HC, WC, c)).astype(dtype)


def _ptrs(m):
    return [int(m.c_frames.data[i] or 0) for i in range(m.n)]


def _geometry(m):
    f = m.c_frames
    return (f.n, f.width, f.height, f.channels, f.depth, f.location, f.row_stride_bytes)


def _struct_bytes(m):
    return bytes(C.string_at(C.addressof(m.c_frames), C.sizeof(m.c_frames)))


def _parent_marshal(frames):
    """What the marshalling did before it knew row-strided views, for host frames: every frame through
    np.ascontiguousarray, stride 0."""
    frames = list(frames)
    keep = [np.ascontiguousarray(f) for f in frames]
    h, w = keep[0].shape[:2]
    c = keep[0].shape[2] if keep[0].ndim == 3 else 1
    return keep, [a.ctypes.data for a in keep], (len(keep), w, h, c, keep[0].dtype.itemsize * 8, HOST, 0)


@pytest.mark.parametrize("dtype,c", [(np.uint8, 3), (np.uint16, 3), (np.float32, 3), (np.uint8, 4), (np.uint8, 1), (np.float32, 1)])
def test_window_of_a_canvas_is_passed_in_place(dtype, c):
    canvas = _canvas(dtype, c)
    el = canvas.itemsize
    win = canvas[:, Y0:Y0 + H, X0:X0 + W, :]
    for frames in (win, list(win), [canvas[i, Y0:Y0 + H, X0:X0 + W] for i in range(N)]):
        m = _Marshalled(frames)
        assert _geometry(m) == (N, W, H, c, el * 8, HOST, WC * c * el)
        base = canvas.ctypes.data + (Y0 * WC + X0) * c * el
        assert _ptrs(m) == [base + i * canvas.strides[0] for i in range(N)]          # an arithmetic progression: no copy
        assert _ptrs(m)[1] - _ptrs(m)[0] != m.c_frames.row_stride_bytes * H           # whose step is not stride * h
        assert len(m.keep) == N
        for k, f in zip(m.keep, win):                                                 # the owners are views of the canvas itself
            assert np.shares_memory(k, canvas) and k.ctypes.data == f.ctypes.data
    if c == 1:                                                                        # h x w frames (no channel axis)
        m = _Marshalled([canvas[i, Y0:Y0 + H, X0:X0 + W, 0] for i in range(N)])
        assert _geometry(m) == (N, W, H, 1, el * 8, HOST, WC * el) and _ptrs(m)[0] == canvas.ctypes.data + (Y0 * WC + X0) * el


def test_windows_at_uneven_places_share_one_stride():
    canvas = _canvas()
    ys = [0, 7, 2, 9]
    m = _Marshalled([canvas[0, y:y + H, X0:X0 + W] for y in ys])
    assert m.c_frames.row_stride_bytes == WC * 3
    assert _ptrs(m) == [canvas.ctypes.data + (y * WC + X0) * 3 for y in ys]
    d = np.diff(_ptrs(m))
    assert len(set(d.tolist())) > 1


def test_padded_rows_and_a_mix_with_contiguous_frames():
    buf = np.zeros((N, H, W * 3 + 5), np.uint8)                                       # an odd stride: 53
    frames = [buf[i, :, :W * 3].reshape(H, W, 3) for i in range(N)]
    assert not frames[0].flags.c_contiguous and np.shares_memory(frames[0], buf)
    m = _Marshalled(frames)
    assert m.c_frames.row_stride_bytes == W * 3 + 5 and _ptrs(m) == [f.ctypes.data for f in frames]
    # a contiguous frame steps its rows by the tight row: with padded frames beside it the strides differ -> copies, stride 0
    tight = np.ascontiguousarray(frames[1])
    m = _Marshalled([frames[0], tight, frames[2]])
    assert m.c_frames.row_stride_bytes == 0
    assert _ptrs(m)[1] == tight.ctypes.data and m.keep[1] is tight                    # the contiguous one stays where it is
    for i in (0, 2):
        assert m.keep[i].flags.c_contiguous and not np.shares_memory(m.keep[i], buf) and _ptrs(m)[i] == m.keep[i].ctypes.data
        assert np.array_equal(m.keep[i], frames[i])


def test_every_other_layout_is_copied():
    canvas = _canvas()
    a = _canvas()[:, :H, :W]
    other = np.zeros((H, W * 3 + 8), np.uint8)[:, :W * 3].reshape(H, W, 3)
    cases = {
        "differing row strides": [canvas[0, :H, :W], other, canvas[2, :H, :W]],
        "negative row stride": [canvas[i, H - 1::-1, :W] for i in range(N)],
        "mirrored columns": [canvas[i, :H, W - 1::-1] for i in range(N)],
        "every second column": [canvas[i, :H, :2 * W:2] for i in range(N)],
        "reversed channels": [canvas[i, :H, :W, ::-1] for i in range(N)],
        "transposed": [np.ascontiguousarray(a[i]).transpose(1, 0, 2)[:H, :H] for i in range(N)],
        "4-D with stepped columns": canvas[:, :H, ::2],
        "element stride below a row (broadcast rows)": [np.broadcast_to(canvas[i, :1, :W], (H, W, 3)) for i in range(N)],
    }
    for name, frames in cases.items():
        frames = list(frames)
        m = _Marshalled(frames)
        assert m.c_frames.row_stride_bytes == 0, name
        for k, f, p in zip(m.keep, frames, _ptrs(m)):
            assert k.flags.c_contiguous and p == k.ctypes.data, name
            assert np.array_equal(k, f), name
            assert f.flags.c_contiguous or not np.shares_memory(k, f), name
    # a 16-bit view whose row step is no whole number of elements
    raw = np.zeros(H * 101 + 8, np.uint8)
    odd = np.lib.stride_tricks.as_strided(raw[:2].view(np.uint16), (H, W, 3), (101, 6, 2), writeable=False)
    m = _Marshalled([odd, odd])
    assert m.c_frames.row_stride_bytes == 0 and all(k.flags.c_contiguous for k in m.keep)


@pytest.mark.parametrize("dtype,c", [(np.uint8, 3), (np.uint16, 3), (np.float32, 3), (np.uint8, 4)])
def test_a_contiguous_stack_is_marshalled_as_before(dtype, c):
    stack = np.ascontiguousarray(_canvas(dtype, c))
    for frames in (stack, list(stack), [stack[i] for i in range(N)], [f.copy() for f in stack]):
        m = _Marshalled(frames)
        keep, ptrs, geo = _parent_marshal(frames)
        assert _geometry(m) == geo and m.c_frames.row_stride_bytes == 0
        assert _ptrs(m) == ptrs == [f.ctypes.data for f in frames]                    # the caller's own memory
        assert all(k is f or k.ctypes.data == f.ctypes.data for k, f in zip(m.keep, frames))
        # byte for byte the struct the parent built: same fields, the pointer array's contents compared above
        ref = api._ffi.Frames(m.c_frames.data, *geo)
        assert _struct_bytes(m)[C.sizeof(C.c_void_p):] == bytes(C.string_at(C.addressof(ref), C.sizeof(ref)))[C.sizeof(C.c_void_p):]
    # h x w frames, and frames that are contiguous slices of a stack
    m = _Marshalled([stack[i, :, :, 0].copy() for i in range(N)])
    assert _geometry(m)[3] == 1 and m.c_frames.row_stride_bytes == 0
    m = _Marshalled(stack[1:3])
    assert _ptrs(m) == [stack[1].ctypes.data, stack[2].ctypes.data] and m.c_frames.row_stride_bytes == 0


def test_geometry_errors_are_unchanged():
    canvas = _canvas()
    with pytest.raises(InvalidParams):
        _Marshalled([canvas[0, :H, :W], canvas[1, :H, :W + 1]])
    with pytest.raises(InvalidParams):
        _Marshalled([canvas[0, :H, :W].astype(np.int32)] * 2)
    assert _Marshalled([]).n == 0


def test_torch_host_tensors_follow_the_same_rules():
    import torch
    canvas = torch.from_numpy(_canvas())
    win = canvas[:, Y0:Y0 + H, X0:X0 + W, :]
    assert not win.is_contiguous()
    m = _Marshalled(win)
    assert _geometry(m) == (N, W, H, 3, 8, HOST, WC * 3)
    assert _ptrs(m) == [win[i].data_ptr() for i in range(N)] and _ptrs(m)[1] - _ptrs(m)[0] == canvas.stride(0)
    m = _Marshalled(canvas.contiguous()[:, :, :, :])
    assert m.c_frames.row_stride_bytes == 0 and _ptrs(m)[0] == canvas.data_ptr()
    m = _Marshalled(list(win.flip(1)))                                               # (a flip copies in torch: contiguous again)
    assert m.c_frames.row_stride_bytes == 0


def test_padded_images_hand_their_stride_over_and_other_layouts_are_refused():
    """The f32 sum / accumulator images (api._image_stride_bytes): 0 for a contiguous one, the row step of a window, an
    error for any layout that stk_image_f32 cannot describe (it used to be passed on as if it were tightly packed)."""
    big = np.zeros((H + 2, W + 5, 3), np.float32)
    assert api._image_stride_bytes(big) == 0
    assert api._image_stride_bytes(big[1:1 + H, 2:2 + W]) == (W + 5) * 3 * 4
    assert api._image_stride_bytes(np.zeros((H, W + 3), np.float32)[:, :W]) == (W + 3) * 4      # h x w, one channel
    for bad in (big[:, ::2], big[::-1], big[..., ::-1], big.transpose(1, 0, 2)):
        with pytest.raises(InvalidParams, match="row step"):
            api._image_stride_bytes(bad)
