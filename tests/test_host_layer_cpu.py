"""me/host.py: the decisions the engine's Python wrappers share, checked on CPU tensors (no library, no device)."""
import itertools

import pytest
import torch

from languagegroundedsemseg_amd import engine
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
