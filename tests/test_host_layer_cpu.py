"""me/host.py and hipcall.py: the decisions the engine's Python wrappers share, checked on CPU tensors (no library, no device)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from languagegroundedsemseg_amd import engine, hipcall
from languagegroundedsemseg_amd.me import host


def _buf(dtype, cols):
    return torch.zeros(10, cols, dtype=dtype)


@pytest.mark.parametrize("make,c,want", [
    (lambda: _buf(torch.bfloat16, 24), 24, 0),                  # contiguous: nothing to stride over
    (lambda: _buf(torch.bfloat16, 24)[:, 8:16], 8, 24),
    (lambda: _buf(torch.bfloat16, 24)[:, 4:12], 8, 0),          # 8 bytes off the 16-byte grid
    (lambda: _buf(torch.bfloat16, 12)[:, :8], 8, 0),            # 24-byte rows
    (lambda: _buf(torch.float32, 12)[:, 4:8], 4, 12),
    (lambda: _buf(torch.float32, 12)[:, 2:6], 4, 0),
])
def test_rows_in_place(make, c, want):
    t = make()
    got, ld = host.rows_in_place(t, c)
    assert ld == want == host.row_stride(t, c)
    if want:
        assert got is t
    else:                                                       # no stride: a contiguous copy (the tensor itself if it is one)
        assert got.is_contiguous() and torch.equal(got, t) and (got is t) == t.is_contiguous()
    assert host.rows_in_place(None, c) == (None, 0)


def test_relu_mode_of():
    assert [host.relu_mode_of(r, h) for r, h in itertools.product((False, True), (False, True))] == [0, 0, 2, 1]


def _slotted(*shapes):
    """parameters owning consecutive slots of one flat fp32 bucket, as BucketedDDP lays them out"""
    flat = torch.zeros(sum(torch.Size(s).numel() for s in shapes))
    params, off = [], 0
    for s in shapes:
        p = torch.nn.Parameter(torch.ones(s, dtype=torch.bfloat16))
        p._lgs_grad_slot = (flat, off, tuple(s))
        params.append(p)
        off += p.numel()
    return flat, params


def test_sink_adopts_the_bucket_slots():
    flat, (g, b) = _slotted((8,), (8,))
    sink = host.AffineSink(g, b, 8, flat.device)
    assert sink.adopted and [t.data_ptr() for t in sink.bufs] == [flat.data_ptr(), flat[8:].data_ptr()]
    back = sink.returned(torch.bfloat16, need=False)
    assert back[0] is sink.bufs[0] and back[1] is sink.bufs[1] and back[0].dtype == torch.float32
    flat, (w,) = _slotted((3, 4, 8))
    sink = host.WeightSink(w, w.shape, flat.device)
    assert sink.adopted and sink.bufs[0].data_ptr() == flat.data_ptr() and sink.bufs[0].shape == w.shape


def test_sink_never_mixes_slots_and_scratch():
    flat, (g, b) = _slotted((8,), (8,))
    b.grad = torch.zeros_like(b)                    # a second micro-batch: autograd accumulates, the slot is declined
    sink = host.AffineSink(g, b, 8, flat.device)
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    assert not sink.adopted and len(sink.bufs) == 2
    assert all(t.dtype == torch.float32 and t.shape == (8,) and not lo <= t.data_ptr() < hi for t in sink.bufs)


def test_sink_without_slots_is_scratch_cast_on_return():
    g, b = torch.nn.Parameter(torch.ones(8, dtype=torch.bfloat16)), None      # no bucket; beta is not a Parameter
    sink = host.AffineSink(g, b, 8, g.device)
    assert not sink.adopted
    assert sink.returned(torch.bfloat16, need=False) == (None, None)
    sink.bufs[0].fill_(1.5), sink.bufs[1].fill_(-2.0)
    dg, db = sink.returned(torch.bfloat16, need=True)
    assert dg.dtype == db.dtype == torch.bfloat16 and torch.all(dg == 1.5) and torch.all(db == -2.0)
    w = host.WeightSink(torch.nn.Parameter(torch.ones(2, 3)))                 # callers whose engine call allocates the result
    assert not w.adopted and w.bufs is None


def test_memo_asks_once_per_key_and_tuning_epoch(monkeypatch):
    cache, asked = {}, []

    def ask(v):
        return lambda: asked.append(v) or v

    assert host.memo(cache, ("a", 1), ask(0)) == 0 and host.memo(cache, ("a", 1), ask(5)) == 0      # (a cached 0 / False is an answer)
    assert host.memo(cache, ("a", 2), ask(7)) == 7 and host.memo(cache, ("b", 1), ask(8)) == 8
    assert asked == [0, 7, 8]
    monkeypatch.setattr(engine, "TUNING_EPOCH", engine.TUNING_EPOCH + 1)
    assert host.memo(cache, ("a", 1), ask(9)) == 9 and host.memo(cache, ("a", 1), ask(10)) == 9
    assert asked == [0, 7, 8, 9]


def test_memo_starts_over_past_4096_entries():
    cache = {}
    for i in range(4097):
        host.memo(cache, ("k", i), lambda: i)
    assert len(cache) == 4097
    host.memo(cache, ("k", -1), lambda: -1)
    assert len(cache) == 1 and host.memo(cache, ("k", -1), lambda: 0) == -1


@pytest.mark.parametrize("dbg", ["", "skip", "inline"])
@pytest.mark.parametrize("wide_rule", [True, False])
def test_wgrad_placement_truth_table(monkeypatch, dbg, wide_rule):
    monkeypatch.setattr(host, "_DBG_WGRAD", dbg)
    monkeypatch.setattr(host, "_WIDE_WGRAD_INLINE", wide_rule)
    wide = (256, 256, 65536)
    shapes = [wide, (255, 256, 65536), (256, 255, 65536), (256, 256, 65535), (32, 64, 1 << 20)]
    for (cin, cout, rows), inline in itertools.product(shapes, (False, True)):
        assert host.wgrad_placement(False, cin, cout, rows, inline) == "plain"
        want = "skip" if dbg == "skip" else \
            "inline" if (dbg == "inline" or inline or (wide_rule and (cin, cout, rows) == wide)) else "side"
        assert host.wgrad_placement(True, cin, cout, rows, inline) == want, (dbg, wide_rule, cin, cout, rows, inline)


# ------------------------------------------------------------------------------------------ the call layer (hipcall.py)
def test_ptr_is_a_plain_int_and_none_is_null():
    t = torch.zeros(4)
    assert hipcall.ptr(None) is None
    assert type(hipcall.ptr(t)) is int and hipcall.ptr(t) == t.data_ptr()


def test_dtype_code():
    assert hipcall.dtype_code(torch.zeros(1)) == engine.LGS_F32
    assert hipcall.dtype_code(torch.zeros(1, dtype=torch.bfloat16)) == engine.LGS_BF16
    for dt in (torch.float16, torch.int32):
        with pytest.raises(RuntimeError, match="float32 and bfloat16"):
            hipcall.dtype_code(torch.zeros(1, dtype=dt))


@pytest.mark.parametrize("value", [torch.zeros(3), [1.0, 2.0], None])
def test_require_hip_refuses_host_tensors_and_non_tensors(value):
    with pytest.raises(RuntimeError) as e:
        hipcall.require_hip(value, "the bank points")
    assert all(s in str(e.value) for s in ("HIP tensor", "no CPU fallback", "the bank points"))


@pytest.mark.parametrize("v", [0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, -1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1])
def test_i32_i64_wrap_like_c(v):
    assert hipcall.i32(v) == ctypes.c_int32(v).value
    assert hipcall.i64(v) == ctypes.c_int64(v).value


def test_host_offsets():
    n = 7
    assert hipcall.host_offsets([0, n], n) == [0, n]
    for form in ([0, 0, n], np.array([0, 0, n]), torch.tensor([0, 0, n])):
        off = hipcall.host_offsets(form, n)
        assert off == [0, 0, n] and type(off) is list and all(type(v) is int for v in off)
    for bad in ([0], [1, n], [0, n - 1], [0, 5, 3, n]):          # too short, first != 0, last != n, a descending pair
        with pytest.raises(ValueError, match="scene_offsets"):
            hipcall.host_offsets(bad, n)


def _voxelize_batched(points, offsets):
    from languagegroundedsemseg_amd import augment
    return augment.voxelize_batched(points, offsets, np.tile(np.eye(4), (len(offsets) - 1, 1, 1)))


def _nearest_voxel(points, offsets):
    from languagegroundedsemseg_amd import pointcloud
    return pointcloud.nearest_voxel(None, points, offsets)


@pytest.mark.parametrize("call", [_voxelize_batched, _nearest_voxel])
def test_the_device_refusal_comes_before_the_offset_refusal(call):
    """host points AND a bad offset list: both operators refuse the host tensor first (RuntimeError), before they look at the offsets
    (whose ValueError a HIP tensor would get) -- and neither reaches an engine call"""
    with pytest.raises(RuntimeError, match="HIP tensor"):
        call(torch.zeros(5, 3), [0, 4, 2, 5])
