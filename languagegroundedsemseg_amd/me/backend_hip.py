"""HIP backend: the product path.  Every call goes through the C-ABI (include/lgs_engine.h).

Tensors stay owned by torch; the engine borrows raw device pointers for the duration of a call and
enqueues on torch's current HIP stream.  There is no fallback: a CPU tensor or a missing library
raises RuntimeError.
"""
import ctypes
import os
import threading
import weakref

import torch

from .. import engine
from ..hipcall import (device_index, dtype_code as _dtype_code, on_device as _dev, ptr as _ptr, raw_stream as _stream,
                       require_hip as _require_dev, scratch as _ws)
from .kernel import ALL_CONV_RELATIONS
from .. import tuning as _tuning
from . import host as _host
from .host import AffineSink, WeightSink, memo, param_event, row_stride, rows_in_place

_vp = ctypes.c_void_p
_PACKED = None


def get_packed():
    global _PACKED
    if _PACKED is None:
        _PACKED = PackedWeights()
    return _PACKED


_QUERIES = {}     # host.memo of the engine queries that belong to no map


def _bn_ws_bytes(L, n, c):
    return memo(_QUERIES, ("bn_ws", n, c), L.lgs_bn_workspace_bytes, n, c)


def _ask_bn_pair_plan(L, direction, n, c, dt):
    info = engine.NormPairPlanInfo()
    engine.check(L.lgs_bn_pair_plan(direction, n, c, dt, ctypes.byref(info)))
    return int(info.path), int(info.workspace_bytes)


def _bn_pair_plan(L, direction, n, c, dt):
    """-> (path, workspace bytes) of lgs_bn_forward_pair (direction 0) / lgs_bn_backward_pair (1) for this call on the current device;
    path 0 = the engine issues the two single norms and needs their intermediate (res / dres) from the caller"""
    return memo(_QUERIES, ("bn_pair", direction, n, c, dt), _ask_bn_pair_plan, L, direction, n, c, dt)


# input voxels per batch below which weight gradients are not moved to the side stream (LGS_WGRAD_INLINE_BELOW: tuning knob;
# one 145 k-voxel scene per step: 11.2 -> 10.4 ms, the 1.2 M-voxel batch keeps the side stream: 29.9 vs 30.9 ms)
_WGRAD_INLINE_BELOW = _tuning.host("WGRAD_INLINE_BELOW")


def _raw_event(ev, stream):
    """hipEvent_t of a torch event for the engine to record; torch creates the handle at the first record"""
    h = ev.cuda_event
    if not h:
        ev.record(stream)
        h = ev.cuda_event
    return int(h.value if hasattr(h, "value") else h)


# ---- operands the wrappers below prepare the same way
def _int64(t):          # an index operand (labels, sample indices, tables) as the kernels read it
    return t.contiguous().to(torch.int64)


def _grad32(g):         # an optional upstream gradient as the kernels read it; None stays None
    return g.contiguous().float() if g is not None else None


def _contiguous(t):     # an optional operand (a norm's residual); None stays None
    return t.contiguous() if t is not None else None


def _dy_rows(dy, dtype, c):
    """-> (dy, row stride or 0) of a norm backward's gradient: a column slice of a wider row-major tensor (the gradient of one ME.cat
    input) is read in place when it has the features' dtype, anything else is copied.  0 means c; a caller says so itself where it has to."""
    return rows_in_place(dy, c) if dy.dtype == dtype else (dy.contiguous(), 0)


def _partial_rows(n):   # per-workgroup partial rows of lgs_ce_weight_sum / lgs_split_stats: one per 2048 rows, 1 .. 1024
    return max(1, min(1024, (n + 2047) // 2048))


def _empty_batch(x):    # what nn.BatchNorm1d (= MinkowskiBatchNorm's `.bn`) says about batch statistics of nothing
    return ValueError("Expected more than 1 value per channel when training, got input size %s" % (list(x.shape),))


def _sized_then_filled(call, allocate):
    """the engine's two-phase exports: call(None, None, None) answers the sizes into the caller's out-parameters, allocate() makes the
    buffers from them -> (buffers, whether there is anything to fill), call(addresses) fills them -> the buffers"""
    call(None, None, None)
    bufs, fill = allocate()
    if fill:
        call(*[_ptr(b) for b in bufs])
    return bufs


_DESC_FIELDS = [f for f, _ in engine.PackDesc._fields_]


class _PackEntry:
    """one packed weight image: the device buffer, its layout as plain ints (no ctypes pointers: conv modules that own
    entries stay picklable / deep-copyable) and a WEAK reference to the parameter it was packed from"""
    __slots__ = ("buf", "desc", "valid", "param_ref", "__weakref__")

    def __init__(self, buf, desc, param):
        self.buf, self.desc, self.valid, self.param_ref = buf, desc, None, weakref.ref(param)

    def cdesc(self):
        d = engine.PackDesc()
        for f in _DESC_FIELDS:
            setattr(d, f, self.desc[f])
        return d


class PackedWeights:
    """Registry of packed weight images (lgs_conv_pack_desc / lgs_pack_weights_batch).  Every conv module OWNS the
    images of its launch shapes (`_pack_cache` dict on the module, one entry per (direction, layout)); this registry
    only holds them weakly, so a model that is dropped frees its images and is no longer re-packed.  An image is valid
    while (epoch, parameter version, parameter address) are unchanged.  optimiser.step() of FlatSGD -- which updates the
    parameters through the C-ABI, invisible to torch's version counters -- calls repack_all(): ONE launch re-packs every
    live image from the updated weights, so the ~125 per-call pack launches of a step disappear.
    Writes torch's version counter does not see (`p.data.copy_()`, `p.data.uniform_()`, `dist.broadcast(p.data)`, a
    raw-pointer write through the C-ABI) need invalidate(): reset_parameters(), load_state_dict() and BucketedDDP's
    initial broadcast call it; any other `.data` write must be followed by ME.invalidate_packed_weights()."""

    def __init__(self):
        self.entries = weakref.WeakSet()
        self.epoch = 0
        self._table = None          # (device copy of the descriptors, entry list, max_total)
        self._dirty = True
        self.enabled = _tuning.host("PACK_CACHE") != 0

    def invalidate(self):
        """every cached image is re-packed from its parameter on next use"""
        self.epoch += 1

    def lookup(self, cache, km, op, transposed, weight, w32, cin, cout, dt):
        """-> (packed buffer or None, pack_mode)"""
        if not self.enabled or cache is None:
            return None, 0
        d = km.pack_desc(op, transposed, cin, cout, dt)
        if d.bytes == 0:
            return None, 0
        key = (op, int(transposed), dt, d.ncp, d.nbp, d.K, cin, cout, int(d.dtype), int(d.bytes))   # (d.dtype: the image's own layout code)
        ent = cache.get(key)
        if ent is None:
            buf = torch.empty(int(d.bytes), dtype=torch.uint8, device=w32.device)
            desc = {f: getattr(d, f) for f in _DESC_FIELDS}
            desc["packed"], desc["weight"] = buf.data_ptr(), w32.data_ptr()
            ent = _PackEntry(buf, desc, weight)
            cache[key] = ent
            self.entries.add(ent)
            self._dirty = True
        stamp = (self.epoch, weight._version, w32.data_ptr())
        if ent.desc["weight"] != w32.data_ptr():
            ent.desc["weight"] = w32.data_ptr()
            self._dirty = True
        if ent.valid == stamp:
            return ent.buf, 2
        ent.valid = stamp
        return ent.buf, 1

    def repack_all(self):
        """after the parameters changed behind torch's back (FlatSGD): new epoch, one batched re-pack of the live images"""
        self.epoch += 1
        if not self.enabled:
            return
        live = []
        for e in list(self.entries):
            p = e.param_ref()
            if p is not None and p.dtype == torch.float32 and p.is_contiguous() and p.is_cuda:
                live.append((e, p))
        if not live:
            self._table = None
            return
        ids = tuple(id(e) for e, _ in live)
        if self._dirty or self._table is None or self._table[1] != ids or any(e.desc["weight"] != p.data_ptr() for e, p in live):
            for e, p in live:
                e.desc["weight"] = p.data_ptr()
            arr = (engine.PackDesc * len(live))(*[e.cdesc() for e, _ in live])
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone()
            self._table = (host.to(live[0][0].buf.device), ids, max(int(e.desc["total"]) for e, _ in live))
            self._dirty = False
        tab, _, max_total = self._table
        with _dev(tab.device):
            engine.check(engine.lib().lgs_pack_weights_batch(_ptr(tab), len(live), max_total, _stream()))
        for e, p in live:
            e.valid = (self.epoch, p._version, p.data_ptr())


def invalidate_packed_weights():
    """call after writing conv weights behind torch's version counters (`.data` writes, raw-pointer updates).  Recorded ME calls
    that have not run yet (me/deferred.py) read the weights when they execute: they run first, with the weights of their call."""
    from . import deferred as _deferred
    _deferred.flush_all()
    if _PACKED is not None:
        _PACKED.invalidate()


class HipKernelMap:
    def __init__(self, mgr, handle, in_key, out_key, ks):
        self.mgr, self.h, self.in_key, self.out_key, self.ks = mgr, handle, in_key, out_key, ks
        self.K = ks ** 3
        # host.memo of what the engine answers about this map (several layers share a map; the answers depend on knobs: tile
        # configuration, weight-gradient plans, FP32_SPLIT's 6 instead of 4 bytes per packed element)
        self._memo = {}

    def _ws_bytes(self, L, cin, cout, dt, op):
        return memo(self._memo, ("conv_ws", cin, cout, dt, op), L.lgs_conv_workspace_bytes, self.h, cin, cout, dt, op)

    def block_ws_bytes(self, L, kmap1, cin, planes, dt):
        """lgs_block_workspace_bytes of a block on this 3^3 map (kmap1: the 1x1 map of its downsample branch, or None)"""
        return memo(self._memo, ("block_ws", cin, planes, dt, kmap1 is not None),
                    L.lgs_block_workspace_bytes, self.h, kmap1.h if kmap1 is not None else None, cin, planes, dt)

    def can_accumulate(self, cin, cout, dt):
        """does the forward-view dgrad of this launch shape have the accumulating epilogue (lgs_conv_dgrad_accumulate)?"""
        return memo(self._memo, ("can_accumulate", cin, cout, dt), engine.lib().lgs_conv_dgrad_can_accumulate, self.h, 0, cin, cout, dt)

    def _ask_pack_desc(self, op, transposed, cin, cout, dt):
        d = engine.PackDesc()
        engine.check(engine.lib().lgs_conv_pack_desc(self.h, int(op), int(transposed), int(cin), int(cout), int(dt), ctypes.byref(d)))
        return d

    def pack_desc(self, op, transposed, cin, cout, dt):
        """the packed-image layout of a launch shape on this map (lgs_conv_pack_desc)"""
        return memo(self._memo, ("pack_desc", op, transposed, cin, cout, dt), self._ask_pack_desc, op, transposed, cin, cout, dt)

    def export(self):
        L = engine.lib()
        m = ctypes.c_int64(0)

        def allocate():
            k = torch.empty(m.value, dtype=torch.int32, device=self.mgr.device)
            return (k, torch.empty_like(k), torch.empty_like(k)), m.value

        with _dev(self.mgr.device):
            return _sized_then_filled(lambda k, i, o: engine.check(L.lgs_kmap_export(self.h, k, i, o, _stream(), ctypes.byref(m))), allocate)

    def tables(self, bwd=False):
        """-> (nbr [slots, n_pad], out_row [n_pad], mask64 [n_pad / 64]) of one view as the kernels read them (int32 copies; None
        where the view has no such table): lgs_debug_kmap_tables, for tests that compare two build paths exactly"""
        L = engine.lib()
        n_pad, slots, present = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)

        def allocate():
            n, has = n_pad.value, present.value
            mk = lambda bit, *shape: torch.empty(*shape, dtype=torch.int32, device=self.mgr.device) if has & bit else None
            return (mk(1, slots.value, n), mk(2, n), mk(4, n // 64)), True

        with _dev(self.mgr.device):
            return _sized_then_filled(lambda nbr, orow, mask: engine.check(L.lgs_debug_kmap_tables(
                self.h, int(bwd), nbr, orow, mask, _stream(), ctypes.byref(n_pad), ctypes.byref(slots), ctypes.byref(present))), allocate)

    def _rows(self, transposed):
        n_in = self.mgr.map_size(self.in_key)
        n_out = self.mgr.map_size(self.out_key)
        return (n_out, n_in) if transposed else (n_in, n_out)

    def _w32(self, weight):
        """-> (fp32 contiguous weight tensor whose address the engine reads, cin, cout); the usual case (an fp32 contiguous
        parameter) is the parameter itself: only its address and shape are used, no view objects are built"""
        cout = weight.shape[-1]
        if weight.dtype == torch.float32 and weight.is_contiguous():
            return weight, weight.numel() // (self.K * cout), cout
        w = weight.detach().reshape(self.K, -1, cout).contiguous().float()
        return w, w.shape[1], cout

    def conv_forward(self, x, weight, bias, transposed, bn_pivot=None, want_bn_stats=False, pack_cache=None):
        """want_bn_stats: also return the per-tile BatchNorm statistics of the output (None if this launch shape cannot
        produce them) -> (out, (partials [rows, 2, cout], pivot) | None)"""
        _require_dev(x, "features")
        L = engine.lib()
        w, cin, cout = self._w32(weight)
        # the skip half of a zero-copy ME.cat is a column slice of the concat buffer: gathered in place through a row stride
        vec_ok = cin % (8 if x.dtype == torch.bfloat16 else 4) == 0 and cout % 4 == 0
        x, ld = rows_in_place(x, cin) if vec_ok else (x.contiguous(), 0)
        n_in, n_out = self._rows(transposed)
        assert x.shape[0] == n_in and x.shape[1] == cin, (x.shape, n_in, cin)
        dt = _dtype_code(x)
        part = None
        with _dev(x.device):
            out = torch.empty((n_out, cout), dtype=x.dtype, device=x.device)
            ws = _ws(self._ws_bytes(L, cin, cout, dt, 0), x.device)
            b = bias.detach().reshape(-1).contiguous().float() if bias is not None else None
            if want_bn_stats:
                rows = L.lgs_conv_bn_partial_rows(self.h, int(transposed), cout, dt)
                if rows > 0:
                    part = torch.empty((rows, 2, cout), dtype=torch.float32, device=x.device)
            piv = bn_pivot if part is not None else None
            pk, mode = get_packed().lookup(pack_cache, self, 0, transposed, weight, w, cin, cout, dt)
            engine.check(L.lgs_conv_forward(self.h, int(transposed), _ptr(x), cin, _ptr(w), cout, _ptr(b), _ptr(out), dt,
                                            _ptr(ws), _ptr(part), _ptr(piv), _ptr(pk), int(mode), int(ld), _stream()))
        if want_bn_stats:
            return out, ((part, piv) if part is not None else None)
        return out

    def conv_dgrad(self, gout, weight, transposed, pack_cache=None, accumulate_into=None):
        """accumulate_into: a caller-owned contiguous [n_in, cin] tensor t (the gradient of a residual branch); the result is
        t += dgrad, rounded like "dgrad, then add", formed in the kernel epilogue where the launch shape has one
        (lgs_conv_dgrad_accumulate; t itself is returned) and by an add into the fresh dgrad tensor otherwise."""
        L = engine.lib()
        gout = gout.contiguous()
        w, cin, cout = self._w32(weight)
        n_in, n_out = self._rows(transposed)
        assert gout.shape[0] == n_out and gout.shape[1] == cout
        dt = _dtype_code(gout)
        acc = accumulate_into
        fuse = (acc is not None and acc.is_contiguous() and acc.dtype == gout.dtype and tuple(acc.shape) == (n_in, cin)
                and L.lgs_conv_dgrad_can_accumulate(self.h, int(transposed), cin, cout, dt))
        with _dev(gout.device):
            gin = acc if fuse else torch.empty((n_in, cin), dtype=gout.dtype, device=gout.device)
            ws = _ws(self._ws_bytes(L, cin, cout, dt, 1), gout.device)
            pk, mode = get_packed().lookup(pack_cache, self, 1, transposed, weight, w, cin, cout, dt)
            fn = L.lgs_conv_dgrad_accumulate if fuse else L.lgs_conv_dgrad
            engine.check(fn(self.h, int(transposed), _ptr(gout), cout, _ptr(w), cin, _ptr(gin), dt, _ptr(ws), _ptr(pk), int(mode), _stream()))
            if acc is not None and not fuse:
                gin += acc
        return gin

    def conv_wgrad(self, x, gout, transposed, out=None, stream=None):
        """-> grad_weight [K,cin,cout] fp32; written straight into `out` (e.g. a view of a gradient bucket) if given.
        stream: enqueue on this torch stream instead of the current one (the caller has ordered it after the producers of
        x / gout; no stream context switch on the host)"""
        L = engine.lib()
        if stream is not None and (not gout.is_contiguous() or (not x.is_contiguous() and not row_stride(x, x.shape[1]))):
            with torch.cuda.stream(stream):         # rare: a copy is needed, make it on the target stream
                return self.conv_wgrad(x, gout, transposed, out=out)
        gout = gout.contiguous()
        cin, cout = x.shape[1], gout.shape[1]
        # strided input (see conv_forward): only the position-stationary bf16 kernel reads it in place
        ld = row_stride(x, cin) if (x.dtype == torch.bfloat16 and self.ks in (2, 3) and cin % 8 == 0 and cout % 8 == 0) else 0
        dt = _dtype_code(x)
        if ld and not L.lgs_conv_wgrad_supports_stride(self.h, int(transposed), cin, cout, dt, int(ld)):
            ld = 0         # the position-stationary kernel declines this shape: hand the pair-list kernel a contiguous copy
        if not ld and not x.is_contiguous():
            if stream is not None:
                with torch.cuda.stream(stream):
                    return self.conv_wgrad(x, gout, transposed, out=out)
            x = x.contiguous()
        assert gout.dtype == x.dtype
        raw = stream.cuda_stream if stream is not None else _stream()
        with _dev(x.device):
            if out is not None:
                assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == self.K * cin * cout
                gw = out
            else:
                gw = torch.empty((self.K, cin, cout), dtype=torch.float32, device=x.device)
            if out is None and stream is not None:
                gw.record_stream(stream)
            ws = _ws(self._ws_bytes(L, cin, cout, dt, 2), x.device, stream)
            engine.check(L.lgs_conv_wgrad(self.h, int(transposed), _ptr(x), cin, _ptr(gout), cout, _ptr(gw), dt, _ptr(ws),
                                          int(ld), raw))
        return gw


class HipSegmentMap:
    """fine -> coarse segment map of one manager (include/lgs_engine.h, lgs_manager_segment_map)"""

    def __init__(self, mgr, handle, fine_key, coarse_key):
        self.mgr, self.h, self.fine_key, self.coarse_key = mgr, handle, fine_key, coarse_key
        self.n_fine, self.n_coarse = mgr.map_size(fine_key), mgr.map_size(coarse_key)
        self._memo = {}

    def _ws_bytes(self, L, c):
        return memo(self._memo, ("seg_ws", c), L.lgs_seg_workspace_bytes, self.h, c)


class HipManager:
    """One per input batch (ME semantics); owns the coordinate maps and kernel maps on the device."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("the MI355X engine needs a HIP device, got %s (no CPU fallback)" % device)
        self.device = torch.device("cuda", device_index(device))
        h = _vp(None)
        engine.check(engine.lib().lgs_manager_create(self.device.index, ctypes.byref(h)))
        self.h = h
        self._pid = os.getpid()
        self._sizes = {}
        # kernel-map handles are held WEAKLY here (they hold the manager strongly: autograd contexts keep a map -- and
        # through it the manager -- alive until backward has run): no reference cycle, so the manager and its device
        # memory are released by reference counting the moment the step's tensors and graph are gone, with or without
        # the cyclic garbage collector (bench.py disables it inside the timed region)
        self._kmaps = weakref.WeakValueDictionary()
        self._coords = {}

    def __del__(self):
        try:
            # never touch HIP from a forked child (multiprocessing helpers inherit live Python objects: destroying the
            # parent's manager there segfaults)
            if getattr(self, "h", None) and getattr(self, "_pid", None) == os.getpid():
                engine.lib().lgs_manager_destroy(self.h)
            self.h = None
        except Exception:
            pass

    def check(self):
        """device-side consistency flags of this manager's maps (one synchronisation; tests): 0 = consistent"""
        f = ctypes.c_int(0)
        engine.check(engine.lib().lgs_manager_check(self.h, ctypes.byref(f)))
        return f.value

    def insert(self, coords):
        _require_dev(coords, "coordinates")
        L = engine.lib()
        coords = coords.to(torch.int32).contiguous()
        n = coords.shape[0]
        key, nu = ctypes.c_int(0), ctypes.c_int64(0)
        with _dev(self.device):
            ui = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
            inv = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
            engine.check(L.lgs_manager_insert(self.h, _ptr(coords), n, _ptr(ui), _ptr(inv), _stream(), ctypes.byref(key),
                                              ctypes.byref(nu)))
        self._sizes[key.value] = (nu.value, 1)
        # a batch this small is bound by host work (~250 engine calls per step), not by the GPU: its weight gradients go onto the
        # compute stream (no fork / join events, no second stream to feed) -- see me.modules.conv_weight_grad
        self.inline_wgrad = nu.value < _WGRAD_INLINE_BELOW
        return key.value, nu.value, ui[:nu.value], inv[:n]

    def stride2(self, key):
        L = engine.lib()
        ok, n = ctypes.c_int(0), ctypes.c_int64(0)
        with _dev(self.device):
            engine.check(L.lgs_manager_stride2(self.h, key, _stream(), ctypes.byref(ok), ctypes.byref(n)))
        self._sizes[ok.value] = (n.value, self._sizes[key][1] * 2)
        return ok.value

    def parent_of(self, key):
        fk = ctypes.c_int(-1)
        engine.check(engine.lib().lgs_manager_parent_of(self.h, key, ctypes.byref(fk)))
        return fk.value

    def map_size(self, key):
        return self._sizes[key][0]

    def tensor_stride(self, key):
        return self._sizes[key][1]

    def coords(self, key):
        if key not in self._coords:
            n = self.map_size(key)
            with _dev(self.device):
                c = torch.empty((n, 4), dtype=torch.int32, device=self.device)
                engine.check(engine.lib().lgs_manager_get_coords(self.h, key, _ptr(c), _stream()))
            self._coords[key] = c
        return self._coords[key]

    def nearest(self, key, points, scene_offsets, b, batch_base=0, affines=None, anchor=0.5, want_d2=False):
        """rows int64 [M] (and d2 float32 [M], site-frame units squared) of the sites of map `key` nearest to points [M, 3] float32
        (lgs_manager_nearest; no synchronisation).  scene_offsets: device int64 [b + 1]; affines: None or b x 12 host doubles."""
        _require_dev(points, "points")
        _require_dev(scene_offsets, "scene_offsets")
        m = points.shape[0]
        a12 = None
        if affines is not None:
            flat = [float(v) for v in affines]
            if len(flat) != 12 * b:
                raise ValueError("nearest: %d affine values for %d scenes" % (len(flat), b))
            a12 = (ctypes.c_double * len(flat))(*flat)
        with _dev(self.device):
            rows = torch.empty(m, dtype=torch.int64, device=self.device)
            d2 = torch.empty(m, dtype=torch.float32, device=self.device) if want_d2 else None
            engine.check(engine.lib().lgs_manager_nearest(self.h, key, _ptr(points), m, _ptr(scene_offsets), b, int(batch_base), a12,
                                                          float(anchor), _ptr(rows), _ptr(d2), _stream()))
        return rows, d2

    def origin(self):
        """key of the origin map: one row (b, 0, 0, 0) per batch index, ascending (lgs_manager_origin; no synchronisation)"""
        ok, n = ctypes.c_int(0), ctypes.c_int64(0)
        with _dev(self.device):
            engine.check(engine.lib().lgs_manager_origin(self.h, _stream(), ctypes.byref(ok), ctypes.byref(n)))
        self._sizes[ok.value] = (n.value, 0)
        return ok.value

    def segment_map(self, fine_key, coarse_key):
        """segment map fine -> coarse (a stride-2^k descendant or the origin map) for pooling / broadcast (cached)"""
        k = ("seg", fine_key, coarse_key)
        sm = self._kmaps.get(k)
        if sm is None:
            h = _vp(None)
            with _dev(self.device):
                engine.check(engine.lib().lgs_manager_segment_map(self.h, fine_key, coarse_key, _stream(), ctypes.byref(h)))
            sm = HipSegmentMap(self, h, fine_key, coarse_key)
            self._kmaps[k] = sm
        return sm

    kernel_map_relations = ALL_CONV_RELATIONS     # every relation of the engine's classifier (lgs_manager_kernel_map_ex)

    def kernel_map(self, in_key, out_key, ks, dilation=1):
        k = (in_key, out_key, ks, dilation)
        km = self._kmaps.get(k)
        if km is None:
            h = _vp(None)     # the engine caches the map itself: a second request returns the same handle at no cost
            with _dev(self.device):
                engine.check(engine.lib().lgs_manager_kernel_map_ex(self.h, in_key, out_key, ks, dilation, _stream(), ctypes.byref(h)))
            km = HipKernelMap(self, h, in_key, out_key, ks)
            self._kmaps[k] = km
        return km


def _written_by_engine(*tensors):
    """The engine updated these tensors through raw pointers (running statistics, num_batches_tracked): bump their autograd
    version counters so that everything keyed on `_version` -- MinkowskiBatchNorm's cached eval-mode [mean | invstd] vector,
    torch's own saved-tensor checks -- sees the write (host-only, no launch)."""
    for t in tensors:
        if t is not None:
            torch.autograd.graph.increment_version(t)


class HipBackend:
    name = "hip"
    bn_counts_batches = True    # lgs_bn_forward increments num_batches_tracked itself
    # lgs_bn_forward can write its output into a column slice of a wider buffer (zero-copy ME.cat; host knob ZERO_COPY_CAT=0: A/B)
    bn_out_into = _tuning.host("ZERO_COPY_CAT") != 0
    # lgs_conv_forward can emit the following BatchNorm's statistics from its epilogue -- measured SLOWER in the step (31.5 vs 30.9 ms: the epilogue work on every conv costs more than the skipped column reduction saves), so off unless LGS_CONV_BN_STATS=1
    conv_bn_stats = _tuning.host("CONV_BN_STATS") in ("1", "big")
    conv_bn_stats_min_bytes = (24 << 20) if _tuning.host("CONV_BN_STATS") == "big" else 0   # experiment: large outputs only

    def want_conv_bn_stats(self, n_rows, cout, esize):
        return self.conv_bn_stats and n_rows * cout * esize >= self.conv_bn_stats_min_bytes

    def __init__(self):
        self._side = {}
        self._cur = {}
        self._fork = {}

    def new_manager(self, device):
        return HipManager(device)

    def invalidate_packed_weights(self):
        """conv weights were written behind torch's version counters (`.data` writes): re-pack on next use"""
        invalidate_packed_weights()

    def weights_updated(self):
        """the optimiser changed the parameters outside autograd: re-pack every cached weight image in one launch"""
        get_packed().repack_all()

    def current_stream(self, device):
        """torch.cuda.current_stream(device) without its per-call Python cost: Stream objects are cached per raw handle"""
        idx = device_index(device)
        raw = torch._C._cuda_getCurrentRawStream(idx)
        s = self._cur.get((idx, raw))
        if s is None:
            s = self._cur[(idx, raw)] = torch.cuda.current_stream(device)
        return s

    def fork_event(self, device):
        """one reusable event per device for ordering the side stream after the compute stream (record, then wait_event)"""
        idx = device_index(device)
        ev = self._fork.get(idx)
        if ev is None:
            ev = self._fork[idx] = torch.cuda.Event()
        return ev

    def side_stream(self, device):
        """second HIP stream per device: weight gradients run here, concurrently with the dgrad / BN chain (CU-mask
        partitions for it were measured in round 3: 37.8-57.9 vs 29.8 ms per step, removed)"""
        key = device.index if isinstance(device, torch.device) else torch.device(device).index
        if key not in self._side:
            self._side[key] = torch.cuda.Stream(device=device)
        return self._side[key]

    # ---- pooling / global pooling / broadcast: segmented reductions and broadcasts (lgs_seg_*)
    POOL_OPS = {"sum": 0, "avg": 1, "max": 2, "prod": 3}
    BCAST_OPS = {"copy": 0, "scale": 1, "add": 2, "mul": 3, "copy_x": 4}

    def pool_reduce(self, sm, op, x, x2=None):
        """-> (out [n_coarse, C], argmax int32 [n_coarse, C] for max else None).  x: [n_fine, C] (a column slice of a wider
        row-major tensor is read in place); op "prod" reduces x * x2 (x2 the same layout as x)."""
        _require_dev(x, "features")
        L = engine.lib()
        c = x.shape[1]
        assert x.dim() == 2 and x.shape[0] == sm.n_fine, (tuple(x.shape), sm.n_fine)
        if x.stride(1) != 1 or x.stride(0) < c or (x2 is not None and x2.stride() != x.stride()):
            x = x.contiguous()
            x2 = _contiguous(x2)
        if x2 is not None:
            assert x2.shape == x.shape and x2.dtype == x.dtype
        dt = _dtype_code(x)
        with _dev(x.device):
            out = torch.empty((sm.n_coarse, c), dtype=x.dtype, device=x.device)
            amax = torch.empty((sm.n_coarse, c), dtype=torch.int32, device=x.device) if op == "max" else None
            wsb = sm._ws_bytes(L, c)
            ws = _ws(wsb, x.device) if wsb > 0 else None
            engine.check(L.lgs_seg_reduce(sm.h, self.POOL_OPS[op], _ptr(x), _ptr(x2), max(x.stride(0), c), c, _ptr(out), _ptr(amax),
                                          dt, _ptr(ws), _stream()))
        return out, amax

    def pool_broadcast(self, sm, op, g, x=None, out=None, col=0):
        """fine rows r of coarse row q: out[r] = g[q] ("copy"), g[q] / rows of q ("scale"), x[r] + g[q] ("add"), x[r] * g[q]
        ("mul"), x[r] ("copy_x").  out: a [n_fine, >= col + C] tensor to write columns [col, col + C) of (default: a new one)."""
        src = x if op == "copy_x" else g
        _require_dev(src, "features")
        L = engine.lib()
        c = src.shape[1]
        if g is not None:
            g = g.contiguous()
            assert g.shape[0] == sm.n_coarse, (tuple(g.shape), sm.n_coarse)
        if x is not None:
            if x.stride(1) != 1 or x.stride(0) < c:
                x = x.contiguous()
            assert x.shape[0] == sm.n_fine and x.shape[1] == c, (tuple(x.shape), sm.n_fine, c)
        dt = _dtype_code(src)
        with _dev(src.device):
            if out is None:
                out = torch.empty((sm.n_fine, c), dtype=src.dtype, device=src.device)
            assert out.is_contiguous() and out.shape[0] == sm.n_fine and out.shape[1] >= col + c and out.dtype == src.dtype
            dst = out.data_ptr() + col * out.element_size()
            engine.check(L.lgs_seg_broadcast(sm.h, self.BCAST_OPS[op], _ptr(g), c, _ptr(x), x.stride(0) if x is not None else c,
                                             dst, out.shape[1], dt, _stream()))
        return out

    def pool_max_backward(self, sm, dy, amax):
        """dx [n_fine, C]: dy of each coarse row goes to the fine row that won its max, per channel"""
        _require_dev(dy, "gradient")
        dy = dy.contiguous()
        c = dy.shape[1]
        with _dev(dy.device):
            dx = torch.empty((sm.n_fine, c), dtype=dy.dtype, device=dy.device)
            engine.check(engine.lib().lgs_seg_max_backward(sm.h, _ptr(dy), _ptr(amax), c, _ptr(dx), _dtype_code(dy), _stream()))
        return dx

    # ---- instance norm: per-scene statistics over the origin segment map (lgs_in_*)
    @staticmethod
    def instance_norm_enabled():
        """tuning knob INSTANCE_NORM, read at call time (0 = the torch lines, also on HIP tensors)"""
        return engine.tuning_get("INSTANCE_NORM") != 0

    def instance_norm_forward(self, sm, x, weight, bias, eps):
        """-> (y [n, C] in x's dtype, stats fp32 [n_seg, 2C] = mean, rstd per scene).  sm: the origin segment map of x's map;
        weight, bias: fp32 [C] (or [1, C]) contiguous."""
        _require_dev(x, "features")
        L = engine.lib()
        n, c = x.shape
        assert x.is_contiguous() and n == sm.n_fine, (tuple(x.shape), x.stride(), sm.n_fine)
        assert weight.dtype == torch.float32 and bias.dtype == torch.float32 and weight.numel() == c and bias.numel() == c
        with _dev(x.device):
            y = torch.empty_like(x)
            stats = torch.empty((sm.n_coarse, 2 * c), dtype=torch.float32, device=x.device)
            ws = _ws(L.lgs_in_workspace_bytes(sm.h, c), x.device)
            engine.check(L.lgs_in_forward(sm.h, _ptr(x), c, _ptr(weight), _ptr(bias), float(eps), _ptr(y), _ptr(stats), _dtype_code(x),
                                          _ptr(ws), _stream()))
        _written_by_engine(y, stats)
        return y, stats

    def instance_norm_backward(self, sm, x, dy, weight, stats):
        """-> (dx [n, C] in x's dtype, dweight fp32 [C], dbias fp32 [C]); y is not needed: xhat is recomputed from x and stats"""
        L = engine.lib()
        n, c = x.shape
        assert dy.shape == x.shape and dy.dtype == x.dtype and dy.is_contiguous() and x.is_contiguous()
        with _dev(x.device):
            dx = torch.empty_like(x)
            dweight = torch.empty(c, dtype=torch.float32, device=x.device)
            dbias = torch.empty(c, dtype=torch.float32, device=x.device)
            ws = _ws(L.lgs_in_workspace_bytes(sm.h, c), x.device)
            engine.check(L.lgs_in_backward(sm.h, _ptr(x), _ptr(dy), c, _ptr(weight), _ptr(stats), _ptr(dx), _ptr(dweight), _ptr(dbias),
                                           _dtype_code(x), _ptr(ws), _stream()))
        _written_by_engine(dx, dweight, dbias)
        return dx, dweight, dbias

    # ---- fused BN(+residual)(+ReLU): lgs_bn_forward / lgs_bn_backward
    def bn_forward(self, x, gamma, beta, eps, momentum, running_mean, running_var, residual, relu, num_batches_tracked=None,
                   conv_stats=None, out_into=None):
        """conv_stats = (partials, pivot) from conv_forward(want_bn_stats=True): the statistics pass over x is skipped.
        out_into = (buffer [n, C_total], column offset): y is written straight into that column slice (zero-copy ME.cat)
        and returned as a strided view of the buffer."""
        _require_dev(x, "features")
        L = engine.lib()
        x = x.contiguous()
        n, c = x.shape
        if n == 0:
            raise _empty_batch(x)
        dt = _dtype_code(x)
        part, piv = conv_stats if conv_stats is not None else (None, None)
        with _dev(x.device):
            y, y_ld = self._y_out(x, out_into)
            stats = torch.empty(2 * c, dtype=torch.float32, device=x.device)
            res = _contiguous(residual)
            ws = _ws(_bn_ws_bytes(L, n, c), x.device)
            engine.check(L.lgs_bn_forward(_ptr(x), n, c, _ptr(gamma), _ptr(beta), float(eps), float(momentum),
                                          _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), _ptr(res), int(relu), _ptr(y),
                                          _ptr(stats), dt, _ptr(ws), _ptr(part), int(part.shape[0]) if part is not None else 0,
                                          _ptr(piv), int(y_ld), _stream()))
        _written_by_engine(running_mean, running_var, num_batches_tracked)
        return y, stats

    def bn_backward(self, x, y, dy, gamma, beta, stats, relu, want_residual, dgamma_out=None, dbeta_out=None):
        """relu: 0 none, 1 mask from y, 2 mask recomputed from x (y may be None)"""
        L = engine.lib()
        n, c = x.shape
        dt = _dtype_code(x)
        # a column slice of a wider row-major tensor (the gradient of one ME.cat input) is read in place; the engine is given
        # dy's row stride explicitly, also when it is c
        dy, dy_ld = _dy_rows(dy, x.dtype, c)
        dy_ld = dy_ld or c
        y, y_ld = rows_in_place(y, c)
        with _dev(x.device):
            dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            dres = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_residual else None
            dgamma = dgamma_out if dgamma_out is not None else torch.empty(c, dtype=torch.float32, device=x.device)
            dbeta = dbeta_out if dbeta_out is not None else torch.empty(c, dtype=torch.float32, device=x.device)
            ws = _ws(_bn_ws_bytes(L, n, c), x.device)
            engine.check(L.lgs_bn_backward(_ptr(x), _ptr(y), _ptr(dy), int(dy_ld), n, c, _ptr(gamma), _ptr(beta), _ptr(stats), int(relu), _ptr(dx),
                                           _ptr(dres), _ptr(dgamma), _ptr(dbeta), dt, _ptr(ws), int(y_ld), _stream()))
        return dx, dres, dgamma, dbeta

    # ---- the two norms that meet at a residual add, on shared passes: lgs_bn_forward_pair / lgs_bn_backward_pair
    @staticmethod
    def _bn_params(m, gamma, beta):
        return engine.BnParams(_ptr(gamma), _ptr(beta), _ptr(m.running_mean), _ptr(m.running_var), _ptr(m.num_batches_tracked),
                               float(m.eps), float(m.momentum))

    def bn_forward_pair(self, xa, bn_a, gamma_a, beta_a, xb, bn_b, gamma_b, beta_b, relu, want_res=False):
        """y = relu?(bn_a(xa) + bn_b(xb)) -> y, stats_a, stats_b, res.  bn_a / bn_b: the nn.BatchNorm1d modules (running statistics,
        eps, momentum).  res = bn_b(xb) only when want_res, or when the engine runs the two single norms (then it is their
        intermediate); otherwise None -- lgs_bn_apply on xb and stats_b gives it to a caller that wants it later."""
        _require_dev(xa, "features")
        L = engine.lib()
        xa, xb = xa.contiguous(), xb.contiguous()
        n, c = xa.shape
        if n == 0:
            raise _empty_batch(xa)
        dt = _dtype_code(xa)
        with _dev(xa.device):
            path, wsb = _bn_pair_plan(L, 0, n, c, dt)
            y = torch.empty_like(xa)
            res = torch.empty_like(xa) if (want_res or path == 0) else None
            st = torch.empty((2, 2 * c), dtype=torch.float32, device=xa.device)
            pa, pb = self._bn_params(bn_a, gamma_a, beta_a), self._bn_params(bn_b, gamma_b, beta_b)
            ws = _ws(wsb, xa.device)
            engine.check(L.lgs_bn_forward_pair(_ptr(xa), ctypes.byref(pa), _ptr(st[0]), _ptr(xb), ctypes.byref(pb), _ptr(st[1]), n, c, int(relu),
                                               _ptr(y), 0, _ptr(res), dt, _ptr(ws), _stream()))
        _written_by_engine(bn_a.running_mean, bn_a.running_var, bn_a.num_batches_tracked, bn_b.running_mean, bn_b.running_var,
                           bn_b.num_batches_tracked)
        return y, st[0], st[1], res

    def bn_backward_pair(self, xa, ya, gamma_a, beta_a, stats_a, relu, xb, gamma_b, stats_b, dy, want_residual=False, grads_out=None):
        """both norms receive dy masked by norm a's ReLU -> dxa, dxb, dres (None unless asked for or needed by the engine),
        (dgamma_a, dbeta_a, dgamma_b, dbeta_b); grads_out: four fp32 [c] buffers to write those into"""
        L = engine.lib()
        n, c = xa.shape
        dt = _dtype_code(xa)
        dy, dy_ld = _dy_rows(dy, xa.dtype, c)
        dy_ld = dy_ld or c
        ya, ya_ld = rows_in_place(ya, c)
        with _dev(xa.device):
            path, wsb = _bn_pair_plan(L, 1, n, c, dt)
            dx = torch.empty((2,) + tuple(xa.shape), dtype=xa.dtype, device=xa.device)
            dres = torch.empty(xa.shape, dtype=xa.dtype, device=xa.device) if (want_residual or path == 0) else None
            if grads_out is None:
                g = torch.empty((4, c), dtype=torch.float32, device=xa.device)
                grads_out = (g[0], g[1], g[2], g[3])
            ws = _ws(wsb, xa.device)
            engine.check(L.lgs_bn_backward_pair(_ptr(xa), _ptr(ya), _ptr(gamma_a), _ptr(beta_a), _ptr(stats_a), int(relu), _ptr(xb), _ptr(gamma_b),
                                                _ptr(stats_b), _ptr(dy), int(dy_ld), n, c, _ptr(dx[0]), _ptr(dx[1]), _ptr(grads_out[0]),
                                                _ptr(grads_out[1]), _ptr(grads_out[2]), _ptr(grads_out[3]), _ptr(dres), dt, _ptr(ws), int(ya_ld),
                                                _stream()))
        return dx[0], dx[1], dres, tuple(grads_out)

    # ---- a whole BasicBlock per call (csrc/lgs_block.hip): small batches, everything on the compute stream
    # host staging of lgs_block_fwd / lgs_block_bwd: one buffer per direction and THREAD (ctypes releases the GIL during the call,
    # so a second Python / autograd thread -- multi-device backward, two models driven from two threads -- must not be able to
    # overwrite the struct the engine is still reading; advisor, round 4)
    _blk_tls = threading.local()

    @classmethod
    def _blk_stage(cls, which):
        """-> (buffer, address) of this thread's staging struct for direction `which` ("f" / "b")"""
        st = getattr(cls._blk_tls, which, None)
        if st is None:
            buf = ctypes.create_string_buffer(512)
            st = (buf, ctypes.addressof(buf))
            setattr(cls._blk_tls, which, st)
        return st

    def _block_ws(self, L, kmap3, kmap1, cin, planes, dt, n, device):
        b = kmap3.block_ws_bytes(L, kmap1, cin, planes, dt)
        # conv scratch and BatchNorm scratch are never live at the same time inside the sequence (as in the call-by-call path,
        # where both are the stream's one grow-only buffer): one buffer, sized for the larger
        # (a block with a downsample branch runs two of its norms as a pair: lgs_bn_pair_workspace_bytes)
        return _ws(max(b, _bn_pair_plan(L, 0, n, planes, dt)[1] if kmap1 is not None else _bn_ws_bytes(L, n, planes)), device)

    def block_forward(self, x, kmap3, kmap1, ws3, pcs, norms, affines, relu_final):
        """BasicBlock forward through lgs_block_forward -> (o1, st1, y1, o2, st2, y2, od, std).  The argument struct is packed
        with ONE struct.pack_into call (setting ~50 ctypes fields one by one cost 60 us per block, more than the calls it saves)"""
        L = engine.lib()
        self.block_calls = getattr(self, "block_calls", 0) + 1
        w1, w2, wd = ws3
        n, cin = x.shape
        planes = w1.shape[2]
        dt = _dtype_code(x)
        dev = x.device
        ds = wd is not None
        pk = get_packed()
        with _dev(dev):
            # the branch norm's output is formed only where the engine runs the norms as single calls (lgs_bn_pair_plan: path 0)
            want_res = ds and _bn_pair_plan(L, 0, n, planes, dt)[0] == 0
            buf = torch.empty(((6 if want_res else 5) if ds else 4, n, planes), dtype=x.dtype, device=dev)
            st = torch.empty((3 if ds else 2, 2 * planes), dtype=torch.float32, device=dev)
            p1, pm1 = pk.lookup(pcs[0], kmap3, 0, False, w1, w1, cin, planes, dt)
            p2, pm2 = pk.lookup(pcs[1], kmap3, 0, False, w2, w2, planes, planes, dt)
            pd, pmd = pk.lookup(pcs[2], kmap1, 0, False, wd, wd, cin, planes, dt) if ds else (None, 0)
            b0 = buf.data_ptr()
            row = n * planes * x.element_size()
            s0 = st.data_ptr()
            srow = 2 * planes * 4
            bn = []
            touched = []
            for m, (g, b) in zip(norms, affines):
                if m is None:
                    bn += [0, 0, 0, 0, 0, 0.0, 0.0]
                    continue
                bn += [g.data_ptr(), b.data_ptr(), _ptr(m.running_mean) or 0, _ptr(m.running_var) or 0, _ptr(m.num_batches_tracked) or 0,
                       float(m.eps), float(m.momentum)]
                touched += [m.running_mean, m.running_var, m.num_batches_tracked]
            cws = self._block_ws(L, kmap3, kmap1, cin, planes, dt, n, dev).data_ptr()
            args, addr = self._blk_stage("f")
            engine.BLOCK_FWD_PACK.pack_into(
                args, 0, kmap3.h.value, kmap1.h.value if ds else 0, dt, int(relu_final), cin, planes, n, x.data_ptr(),
                w1.data_ptr(), w2.data_ptr(), wd.data_ptr() if ds else 0,
                _ptr(p1) or 0, _ptr(p2) or 0, _ptr(pd) or 0, int(pm1), int(pm2), int(pmd), *bn,
                b0, b0 + row, b0 + 2 * row, (b0 + 4 * row) if ds else 0, (b0 + 5 * row) if want_res else 0, b0 + 3 * row,
                s0, s0 + srow, (s0 + 2 * srow) if ds else 0, cws, cws)
            engine.check(L.lgs_block_forward(addr, _stream()))
        _written_by_engine(*touched)
        return buf[0], st[0], buf[1], buf[2], st[1], buf[3], (buf[4] if ds else None), (st[2] if ds else None)

    def block_backward(self, dy, saved, extra, kmap3, kmap1, pcs, params, relu_final, want_gin):
        """BasicBlock backward through lgs_block_backward -> the gradient tuple of models._BasicBlockFunction"""
        L = engine.lib()
        self.block_calls = getattr(self, "block_calls", 0) + 1
        x, w1, g1, b1, w2, g2, b2, o1, st1, y1, o2, st2, y2 = saved
        wd, gd, bd, od, std = extra
        pw1, pg1, pb1, pw2, pg2, pb2, pwd, pgd, pbd = params
        n, cin = x.shape
        planes = w1.shape[2]
        dt = _dtype_code(x)
        dev = x.device
        ds = wd is not None
        dy, dy_ld = _dy_rows(dy, x.dtype, planes)      # (no `or planes` here: lgs_block_bwd.dy_row_stride is handed the 0, which means planes)
        pk = get_packed()
        with _dev(dev):
            p1, pm1 = pk.lookup(pcs[0], kmap3, 1, False, w1, w1, cin, planes, dt)
            p2, pm2 = pk.lookup(pcs[1], kmap3, 1, False, w2, w2, planes, planes, dt)
            pd, pmd = pk.lookup(pcs[2], kmap1, 1, False, wd, wd, cin, planes, dt) if ds else (None, 0)
            # the masked gradient is formed only where something reads it: blocks without a branch (it is the residual's gradient),
            # or norms that run as single calls (lgs_bn_pair_plan: path 0)
            want_dres = (not ds) or _bn_pair_plan(L, 1, n, planes, dt)[0] == 0
            buf = torch.empty((5 if want_dres else 4, n, planes) if ds else (4, n, planes), dtype=x.dtype, device=dev)
            b0 = buf.data_ptr()
            row = n * planes * x.element_size()
            b_dres, b_dy1, b_dx1, b_dxd = (b0 + row, b0 + 2 * row, b0 + 3 * row, (b0 + 4 * row) if ds else 0) if want_dres else \
                (0, b0 + row, b0 + 2 * row, b0 + 3 * row)
            sw1, sw2 = WeightSink(pw1, w1.shape, dev), WeightSink(pw2, w2.shape, dev)
            (gw1,), (gw2,) = sw1.bufs, sw2.bufs
            dg1, db1 = AffineSink(pg1, pb1, planes, dev).bufs
            dg2, db2 = AffineSink(pg2, pb2, planes, dev).bufs
            slots = sw1.adopted and sw2.adopted
            gwd = dgd = dbd = gind = None
            if ds:
                swd = WeightSink(pwd, wd.shape, dev)
                (gwd,), slots = swd.bufs, slots and swd.adopted
                dgd, dbd = AffineSink(pgd, pbd, planes, dev).bufs
                gind = torch.empty((n, cin), dtype=x.dtype, device=dev)
            cws = self._block_ws(L, kmap3, kmap1, cin, planes, dt, n, dev).data_ptr()
            # weight gradients beside the dgrad / BatchNorm chain (what modules.conv_weight_grad does call by call): every kernel
            # parameter owns a gradient-bucket slot and the batch is not one of the small ones that keep them on the compute stream
            # (how this differs from the call-by-call rule: host.wgrad_placement)
            side = None
            s_raw = s_ws = s_fork = e1 = e2 = ed = 0
            if not getattr(kmap3.mgr, "inline_wgrad", False) and slots and _host._DBG_WGRAD == "":
                side = self.side_stream(dev)
                s_raw = side.cuda_stream
                need = max(kmap3._ws_bytes(L, cin, planes, dt, 2), kmap3._ws_bytes(L, planes, planes, dt, 2),
                           kmap1._ws_bytes(L, cin, planes, dt, 2) if ds else 0)
                s_ws = _ws(need, dev, side).data_ptr()
                s_fork = _raw_event(self.fork_event(dev), side)
                e1, e2 = _raw_event(param_event(pw1), side), _raw_event(param_event(pw2), side)
                ed = _raw_event(param_event(pwd), side) if ds else 0
            args_b, addr_b = self._blk_stage("b")
            engine.BLOCK_BWD_PACK.pack_into(
                args_b, 0, kmap3.h.value, kmap1.h.value if ds else 0, dt, int(relu_final), cin, planes, int(want_gin), 0,
                n, dy_ld, dy.data_ptr(),
                x.data_ptr(), o1.data_ptr(), y1.data_ptr(), o2.data_ptr(), y2.data_ptr() if relu_final else 0, od.data_ptr() if ds else 0,
                st1.data_ptr(), st2.data_ptr(), std.data_ptr() if ds else 0,
                w1.data_ptr(), w2.data_ptr(), wd.data_ptr() if ds else 0,
                _ptr(p1) or 0, _ptr(p2) or 0, _ptr(pd) or 0, int(pm1), int(pm2), int(pmd),
                g1.data_ptr(), b1.data_ptr(), g2.data_ptr(), b2.data_ptr(), gd.data_ptr() if ds else 0, bd.data_ptr() if ds else 0,
                b0, b_dres, b_dy1, b_dx1, b_dxd, gind.data_ptr() if ds else 0,
                gw1.data_ptr(), gw2.data_ptr(), gwd.data_ptr() if ds else 0,
                dg1.data_ptr(), db1.data_ptr(), dg2.data_ptr(), db2.data_ptr(), dgd.data_ptr() if ds else 0, dbd.data_ptr() if ds else 0,
                cws, cws, s_raw, s_ws, s_fork, e1, e2, ed)
            engine.check(L.lgs_block_backward(addr_b, _stream()))
            if side is not None:
                # (parameters in the order the engine issued them; the side stream reads the operands after this call returns)
                _host.side_wgrads_issued(side, (pw2, pw1, pwd) if ds else (pw2, pw1), (x, y1, buf))
        gin = (gind if ds else buf[1]) if want_gin else None
        # (all parameters of the fast path are fp32: the engine's fp32 gradients need no cast)
        out = (gin, None, None, None, gw1, dg1, db1, gw2, dg2, db2)
        if ds:
            out = out + (gwd, dgd, dbd)
        return out

    # ---- the same op in halves (SyncBN: statistics are exchanged between ranks in the middle)
    def bn_stats(self, x, conv_stats=None):
        """-> float32 [2C+1]: local mean, local M2, row count (the record one rank contributes to SyncBN's all-gather)"""
        L = engine.lib()
        x = x.contiguous()
        n, c = x.shape
        part, piv = conv_stats if conv_stats is not None else (None, None)
        with _dev(x.device):
            out = torch.empty(2 * c + 1, dtype=torch.float32, device=x.device)
            ws = _ws(_bn_ws_bytes(L, n, c), x.device)
            engine.check(L.lgs_bn_stats(_ptr(x), n, c, _ptr(out), _dtype_code(x), _ptr(ws), _ptr(part),
                                        int(part.shape[0]) if part is not None else 0, _ptr(piv), _stream()))
        return out

    def bn_sync_combine(self, all_stats, c, eps, momentum, running_mean, running_var, num_batches_tracked):
        """all_stats [world, 2C+1] -> (stats [2C] = global mean | invstd, inv_n [1] = 1 / global rows); one kernel"""
        L = engine.lib()
        world = all_stats.shape[0]
        with _dev(all_stats.device):
            stats = torch.empty(2 * c, dtype=torch.float32, device=all_stats.device)
            inv_n = torch.empty(1, dtype=torch.float32, device=all_stats.device)
            engine.check(L.lgs_bn_sync_combine(_ptr(all_stats), int(world), int(c), float(eps), float(momentum), _ptr(running_mean),
                                               _ptr(running_var), _ptr(num_batches_tracked), _ptr(stats), _ptr(inv_n), _stream()))
        _written_by_engine(running_mean, running_var, num_batches_tracked)
        return stats, inv_n

    def bn_apply(self, x, gamma, beta, stats, residual, relu, out_into=None):
        L = engine.lib()
        x = x.contiguous()
        n, c = x.shape
        with _dev(x.device):
            y, y_ld = self._y_out(x, out_into)
            if n == 0:                     # an empty batch (a zero-row tensor has no storage to point at): nothing to normalise
                return y
            res = _contiguous(residual)
            engine.check(L.lgs_bn_apply(_ptr(x), n, c, _ptr(gamma), _ptr(beta), _ptr(stats), _ptr(res), int(relu), _ptr(y),
                                        _dtype_code(x), int(y_ld), _stream()))
        return y

    # ---- SyncBN as one call per direction on the engine's own RCCL communicator (csrc/lgs_comm.hip)
    @staticmethod
    def _y_out(x, out_into):
        """-> (y, row stride for the engine): a fresh tensor, or the column slice of a concat buffer (zero-copy ME.cat)"""
        if out_into is None:
            return torch.empty_like(x), 0
        buf, off = out_into
        n, c = x.shape
        y = buf[:, off:off + c]
        ld = row_stride(y, c)
        assert buf.dtype == x.dtype and buf.shape[0] == n and ld, (tuple(buf.shape), buf.dtype, off, c)
        return y, ld

    def bn_forward_sync(self, comm, x, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, residual, relu,
                        out_into=None):
        """-> y, stats [2C], inv_n [1]"""
        L = engine.lib()
        x = x.contiguous()
        n, c = x.shape
        with _dev(x.device):
            y, y_ld = self._y_out(x, out_into)
            stats = torch.empty(2 * c + 1, dtype=torch.float32, device=x.device)      # [mean | invstd | 1 / global rows]
            res = _contiguous(residual)
            ws = _ws(L.lgs_bn_sync_workspace_bytes(n, c, comm.world), x.device)
            engine.check(L.lgs_bn_forward_sync(comm.h, _ptr(x), n, c, _ptr(gamma), _ptr(beta), float(eps), float(momentum),
                                               _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), _ptr(res), int(relu),
                                               _ptr(y), stats.data_ptr(), stats.data_ptr() + 8 * c, _dtype_code(x), _ptr(ws), int(y_ld), _stream()))
        _written_by_engine(running_mean, running_var, num_batches_tracked)
        return y, stats[:2 * c], stats[2 * c:]

    def bn_backward_sync(self, comm, x, y, dy, gamma, beta, stats, inv_n, relu, want_residual, dgamma_out=None, dbeta_out=None):
        """-> dx, dres (dgamma_out / dbeta_out receive the LOCAL parameter gradients)"""
        L = engine.lib()
        n, c = x.shape
        dy, dy_ld = rows_in_place(dy, c)
        y, y_ld = rows_in_place(y, c)
        with _dev(x.device):
            dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            dres = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_residual else None
            ws = _ws(L.lgs_bn_sync_workspace_bytes(n, c, comm.world), x.device)
            engine.check(L.lgs_bn_backward_sync(comm.h, _ptr(x), _ptr(y), _ptr(dy), n, c, _ptr(gamma), _ptr(beta), _ptr(stats), _ptr(inv_n),
                                                int(relu), _ptr(dx), _ptr(dres), _ptr(dgamma_out), _ptr(dbeta_out), _dtype_code(x),
                                                _ptr(ws), int(dy_ld), int(y_ld), _stream()))
        return dx, dres

    def bn_backward_reduce(self, x, y, dy, gamma, beta, stats, relu, dgamma_out=None, dbeta_out=None):
        """-> sums [2C] (local sum dy', sum dy' xhat); the same vectors are also written to dgamma_out / dbeta_out"""
        L = engine.lib()
        n, c = x.shape
        dy, dy_ld = rows_in_place(dy, c)
        y, y_ld = rows_in_place(y, c)
        with _dev(x.device):
            if n == 0:                     # empty batch: zero sums (and zero parameter gradients)
                for t in (dgamma_out, dbeta_out):
                    if t is not None:
                        t.zero_()
                return torch.zeros(2 * c, dtype=torch.float32, device=x.device)
            sums = torch.empty(2 * c, dtype=torch.float32, device=x.device)
            ws = _ws(_bn_ws_bytes(L, n, c), x.device)
            engine.check(L.lgs_bn_backward_reduce(_ptr(x), _ptr(y), _ptr(dy), n, c, _ptr(gamma), _ptr(beta), _ptr(stats), int(relu), _ptr(sums),
                                                  _ptr(dgamma_out), _ptr(dbeta_out), _dtype_code(x), _ptr(ws), int(dy_ld), int(y_ld), _stream()))
        return sums

    def bn_backward_apply(self, x, y, dy, gamma, beta, stats, sums, inv_n_total, relu, want_residual):
        """inv_n_total: python float, or a device scalar tensor (1 / global row count, no host sync)"""
        L = engine.lib()
        n, c = x.shape
        dev_inv = inv_n_total if torch.is_tensor(inv_n_total) else None
        dy, dy_ld = rows_in_place(dy, c)
        y, y_ld = rows_in_place(y, c)
        with _dev(x.device):
            dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            dres = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_residual else None
            if n == 0:
                return dx, dres
            engine.check(L.lgs_bn_backward_apply(_ptr(x), _ptr(y), _ptr(dy), n, c, _ptr(gamma), _ptr(beta), _ptr(stats), _ptr(sums),
                                                 0.0 if dev_inv is not None else float(inv_n_total), _ptr(dev_inv), int(relu), _ptr(dx),
                                                 _ptr(dres), _dtype_code(x), int(dy_ld), int(y_ld), _stream()))
        return dx, dres

    # ---- CLIP contraction: lgs_clip_similarity
    def clip_similarity(self, feats, anchors):
        _require_dev(feats, "features")
        L = engine.lib()
        feats = feats.contiguous()
        anchors = anchors.detach().contiguous().float()
        n, c = feats.shape
        na = anchors.shape[0]
        dt = _dtype_code(feats)
        with _dev(feats.device):
            sim = torch.empty((n, na), dtype=torch.float32, device=feats.device)
            inv = torch.empty(max(n, 1), dtype=torch.float32, device=feats.device)
            ws = _ws(L.lgs_clip_workspace_bytes(c, na, dt), feats.device)
            engine.check(L.lgs_clip_similarity(_ptr(feats), n, c, _ptr(anchors), na, _ptr(sim), _ptr(inv), dt, _ptr(ws),
                                               _stream()))
        return sim, inv[:n]

    # ---- fused CLIP text-anchor loss: lgs_clip_loss_forward / lgs_clip_loss_backward
    CLIP_LOSS_MAX_ANCHORS = 224

    def clip_loss_forward(self, feats, anchors, labels, neg, ignore_label, want_sim=False):
        """one pass over the features -> (d_pos [N], d_neg [N], pred [N] int64, saved-for-backward tuple, sim or None)"""
        _require_dev(feats, "features")
        L = engine.lib()
        feats = feats.contiguous()
        anchors = anchors.detach().contiguous().float()
        labels = _int64(labels)
        neg = _int64(neg)
        n, c = feats.shape
        na, k = anchors.shape[0], neg.shape[1]
        dt = _dtype_code(feats)
        dev = feats.device
        with _dev(dev):
            d_pos = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
            d_neg = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
            inv = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
            pred = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
            tn = torch.empty((na, c), dtype=torch.float32, device=dev)
            sim = torch.empty((n, na), dtype=torch.float32, device=dev) if want_sim else None
            ws = _ws(L.lgs_clip_loss_workspace_bytes(c, na, dt), dev)
            engine.check(L.lgs_clip_loss_forward(_ptr(feats), n, c, _ptr(anchors), na, _ptr(labels), _ptr(neg), int(k),
                                                 int(ignore_label), _ptr(d_pos), _ptr(d_neg), _ptr(pred), _ptr(inv), _ptr(tn),
                                                 _ptr(sim), dt, _ptr(ws), _stream()))
        return d_pos[:n], d_neg[:n], pred[:n], (feats, tn, labels, neg, inv), sim

    def clip_loss_backward(self, saved, d_pos, d_neg, g_dpos, g_dneg, ignore_label):
        L = engine.lib()
        feats, tn, labels, neg, inv = saved
        n, c = feats.shape
        with _dev(feats.device):
            gf = torch.empty_like(feats)
            gp = _grad32(g_dpos)
            gn = _grad32(g_dneg)
            engine.check(L.lgs_clip_loss_backward(_ptr(feats), n, c, _ptr(tn), tn.shape[0], _ptr(labels), _ptr(neg), int(neg.shape[1]),
                                                  int(ignore_label), _ptr(inv), _ptr(d_pos), _ptr(d_neg), _ptr(gp), _ptr(gn), _ptr(gf),
                                                  _dtype_code(feats), _stream()))
        return gf

    def clip_loss_backward_anchors(self, saved, g_dpos, g_dneg, ignore_label):
        """-> d loss / d t^ [n_anchor, c] float32 (gradient w.r.t. the NORMALISED anchors): lgs_clip_loss_backward_anchors"""
        L = engine.lib()
        feats, tn, labels, neg, inv = saved
        n, c = feats.shape
        na = tn.shape[0]
        a8 = (na + 7) // 8 * 8
        dt = _dtype_code(feats)
        with _dev(feats.device):
            gt = torch.empty((c, a8), dtype=torch.float32, device=feats.device)
            gp = _grad32(g_dpos)
            gn = _grad32(g_dneg)
            ws = _ws(L.lgs_clip_anchor_grad_workspace_bytes(n, c, na, dt), feats.device)
            engine.check(L.lgs_clip_loss_backward_anchors(_ptr(feats), n, c, na, _ptr(labels), _ptr(neg), int(neg.shape[1]),
                                                          int(ignore_label), _ptr(inv), _ptr(gp), _ptr(gn), _ptr(gt), dt, _ptr(ws),
                                                          _stream()))
        return gt[:, :na].t()

    # ---- the class-row losses (csrc/lgs_classrows.h): fused softmax cross-entropy lgs_ce_forward_backward_rows, focal loss /
    # class-weighted cross-entropy lgs_focal_forward_backward
    @staticmethod
    def class_limit(dtype):
        """the widest [N, C] head half a wavefront holds (lgs_classrows.h: 32 lanes x 4 chunks of 16 bytes): 512 classes in fp32, 1024
        in bf16; 0 for a dtype the class-row kernels do not take"""
        return {torch.float32: 512, torch.bfloat16: 1024}.get(dtype, 0)

    def _class_rows(self, logits, labels, ignore_index, focal, want_rows, want_grad, scale=None, row_grad=None):
        """the one launch behind the four loss methods -> (loss_rows [N] fp32 or None, dlogits or None).  focal: None = k_ce_fwd_bwd,
        (alpha, gamma) = k_focal_fwd_bwd.  The gradient is multiplied by scale (device scalar, default 1) and row_grad [N].
        An empty batch gives empty results without a launch."""
        _require_dev(logits, "logits")
        L = engine.lib()
        logits = logits.contiguous()
        labels = _int64(labels)
        n, c = logits.shape
        dev = logits.device
        with _dev(dev):
            loss_rows = torch.empty(n, dtype=torch.float32, device=dev) if want_rows else None
            dlogits = torch.empty_like(logits) if want_grad else None
            if n == 0:
                return loss_rows, dlogits
            row_grad = _grad32(row_grad)
            args = (_ptr(scale if scale is not None else self._one(dev)), _ptr(row_grad), _ptr(loss_rows), _ptr(dlogits),
                    _dtype_code(logits), _stream())
            if focal is None:
                engine.check(L.lgs_ce_forward_backward_rows(_ptr(logits), n, c, _ptr(labels), int(ignore_index), *args))
            else:
                engine.check(L.lgs_focal_forward_backward(_ptr(logits), n, c, _ptr(labels), int(ignore_index), _ptr(focal[0]),
                                                          float(focal[1]), *args))
        return loss_rows, dlogits

    def _class_reduced(self, logits, labels, ignore_index, focal, denom, want_grad, grad_scale, inv_denom):
        """a reduced loss on _class_rows -> (loss or None, dlogits or None, inv_denom).  grad_scale (device scalar): gradient only,
        already multiplied by it.  inv_denom: 1 / the denominator, from an earlier call on the same labels or computed here from
        denom: 'valid' = the counted rows (lgs_ce_count_valid: the kernel's predicate, a label outside [0, C) is an ignored row),
        'weight' = the sum of alpha[label] (ce_weight_sum; a zero sum counts as 1), 'sum' = 1.  An empty batch: loss 0, 1."""
        _require_dev(logits, "logits")
        labels = _int64(labels)
        n, c = logits.shape
        one = self._one(logits.device)
        if inv_denom is None:
            if n == 0 or denom == "sum":
                inv_denom = one
            elif denom == "valid":
                with _dev(logits.device):
                    cnt = torch.empty(1, dtype=torch.int32, device=logits.device)
                    engine.check(engine.lib().lgs_ce_count_valid(_ptr(labels), n, c, int(ignore_index), _ptr(cnt), _stream()))
                inv_denom = cnt.to(torch.float32).clamp_min_(1.0).reciprocal_().reshape(())
            elif denom == "weight":
                s = self.ce_weight_sum(labels, c, ignore_index, focal[0])
                inv_denom = torch.where(s > 0, s, one).reciprocal_()
            else:
                raise ValueError("focal_loss: denom must be 'valid', 'weight' or 'sum'")
        scale = inv_denom if grad_scale is None else inv_denom * grad_scale.to(torch.float32).reshape(())
        loss_rows, dlogits = self._class_rows(logits, labels, ignore_index, focal, grad_scale is None, want_grad or grad_scale is not None,
                                              scale=scale)
        return (loss_rows.sum() * inv_denom if loss_rows is not None else None), dlogits, inv_denom

    def cross_entropy(self, logits, labels, ignore_index, want_grad=True, grad_scale=None, inv_valid=None):
        """mean CE over the non-ignored rows.  want_grad=False: loss only; grad_scale (device scalar): gradient only,
        already multiplied by it (the two halves of one kernel, so the upstream gradient never needs its own pass).
        inv_valid: 1 / #counted rows from an earlier call on the same labels (the forward's, reused by the backward).
        -> (loss, dlogits, inv_valid)"""
        return self._class_reduced(logits, labels, ignore_index, None, "valid", want_grad, grad_scale, inv_valid)

    def cross_entropy_rows(self, logits, labels, ignore_index, row_grad=None):
        """nn.CrossEntropyLoss(reduction='none') (pl_BaselineTrainer.py:94 under balanced_category_sampling): row_grad=None ->
        the per-row losses [N] (0 for ignored rows); row_grad [N] fp32 = the upstream gradient -> d(logits), one pass either way.
        No denominator: the caller's reduction owns it."""
        loss_rows, dlogits = self._class_rows(logits, labels, ignore_index, None, row_grad is None, row_grad is not None, row_grad=row_grad)
        return loss_rows if row_grad is None else dlogits

    def ce_weight_sum(self, labels, n_classes, ignore_index, alpha):
        """sum of alpha[label] over the counted rows -> device scalar (lgs_ce_weight_sum: per-workgroup partials added up in fixed
        order), the denominator of nn.CrossEntropyLoss(weight=alpha) 'mean'.  No host sync."""
        _require_dev(alpha, "alpha")
        L = engine.lib()
        labels = _int64(labels)
        n = labels.shape[0]
        if n == 0:
            return self._one(alpha.device) * 0.0
        rows = _partial_rows(n)
        with _dev(alpha.device):
            partial = torch.empty(rows, dtype=torch.float32, device=alpha.device)
            engine.check(L.lgs_ce_weight_sum(_ptr(labels), n, int(n_classes), int(ignore_index), _ptr(alpha), _ptr(partial), rows, _stream()))
        return partial.sum()

    def focal_loss(self, logits, labels, ignore_index, alpha, gamma, denom="valid", grad_scale=None, inv_denom=None):
        """reduced focal loss -a u^gamma log(pt) (gamma == 0: class-weighted cross-entropy), the two halves of one kernel like
        cross_entropy: grad_scale=None -> the loss; grad_scale (device scalar) -> d(logits), already multiplied by it.
        alpha: [C] fp32 on the device, or None.  denom: 'valid' = mean over the counted rows (FocalLoss 'mean'), 'weight' = over the
        sum of alpha[label] (nn.CrossEntropyLoss(weight) 'mean'), 'sum' = none.  inv_denom: the forward's, reused by the backward.
        -> (loss, dlogits, inv_denom)"""
        return self._class_reduced(logits, labels, ignore_index, (alpha, gamma), denom, False, grad_scale, inv_denom)

    def focal_loss_rows(self, logits, labels, ignore_index, alpha, gamma, row_grad=None):
        """reduction='none': row_grad=None -> the per-row losses [N] fp32 (0 for ignored rows); row_grad [N] = the upstream gradient
        -> d(logits); one pass either way, like cross_entropy_rows."""
        loss_rows, dlogits = self._class_rows(logits, labels, ignore_index, (alpha, gamma), row_grad is None, row_grad is not None,
                                              row_grad=row_grad)
        return loss_rows if row_grad is None else dlogits

    def split_stats(self, loss_rows, labels, group_of_class, ignore_index):
        """-> [3, 2] fp32: (sum of loss_rows, number of rows) of the head / common / tail points (lgs_split_stats), no host sync"""
        _require_dev(loss_rows, "loss_rows")
        L = engine.lib()
        loss_rows = loss_rows.detach().contiguous().to(torch.float32)
        labels = _int64(labels)
        group_of_class = group_of_class.contiguous().to(torch.int32)
        n = loss_rows.shape[0]
        rows = _partial_rows(n)
        with _dev(loss_rows.device):
            partial = torch.empty(rows, 6, dtype=torch.float32, device=loss_rows.device)
            engine.check(L.lgs_split_stats(_ptr(loss_rows), _ptr(labels), n, _ptr(group_of_class), int(group_of_class.shape[0]),
                                           int(ignore_index), _ptr(partial), rows, _stream()))
        return partial.sum(0).view(3, 2)

    # ---- segmentation metrics: lgs_seg_metrics
    @staticmethod
    def seg_metrics_supports(scores):
        """fp32 or bf16 scores of at most class_limit classes"""
        return 1 <= scores.shape[1] <= HipBackend.class_limit(scores.dtype)

    def seg_metrics(self, scores, labels, ignore_index, confmat, want_prob=False):
        """one pass over scores [N, C]: -> (pred [N] int64 = scores.max(1)[1], prob [N, C] fp32 softmax or None); adds the rows with
        a label in [0, C) other than ignore_index to confmat [C, C] (int64, contiguous, accumulated IN PLACE).  No host sync."""
        _require_dev(scores, "scores")
        _require_dev(confmat, "confmat")
        L = engine.lib()
        scores = scores.detach().contiguous()
        labels = _int64(labels)
        n, c = scores.shape
        if confmat.dtype != torch.int64 or tuple(confmat.shape) != (c, c) or not confmat.is_contiguous():
            raise RuntimeError("seg_metrics: confmat must be a contiguous int64 [%d, %d] tensor" % (c, c))
        if labels.shape[0] != n:
            raise RuntimeError("seg_metrics: %d labels for %d rows" % (labels.shape[0], n))
        with _dev(scores.device):
            pred = torch.empty(n, dtype=torch.int64, device=scores.device)
            prob = torch.empty(n, c, dtype=torch.float32, device=scores.device) if want_prob else None
            engine.check(L.lgs_seg_metrics(_ptr(scores), n, c, _ptr(labels), int(ignore_index), _ptr(pred), _ptr(prob), _ptr(confmat),
                                           _dtype_code(scores), _stream()))
        return pred, prob

    # ---- per-class average precision: lgs_average_precision
    @staticmethod
    def average_precision_supports(scores):
        """fp32 or bf16 scores of at most class_limit classes"""
        return scores.dtype in (torch.float32, torch.bfloat16) and 1 <= scores.shape[1] <= HipBackend.class_limit(scores.dtype)

    def average_precision(self, scores, labels, ignore_index, from_logits=False):
        """scores [N, C] -> float64 [C]: sklearn's step-wise AP of every class, NaN for a class without a positive row (the rows with
        a label in [0, C) other than ignore_index are the positives of their class; every other row is a negative of all).
        from_logits: rank the fp32 softmax of the scores -- the very bits seg_metrics' prob holds -- without materialising it.
        Sorted positives, one counting pass over the scores; no host sync."""
        _require_dev(scores, "scores")
        L = engine.lib()
        scores = scores.detach().contiguous()
        labels = _int64(labels)
        n, c = scores.shape
        if labels.shape[0] != n:
            raise RuntimeError("average_precision: %d labels for %d rows" % (labels.shape[0], n))
        with _dev(scores.device):
            ap = torch.empty(c, dtype=torch.float64, device=scores.device)
            ws = None
            if n > 0:
                nbytes = memo(_QUERIES, ("ap_ws", n, c), L.lgs_ap_workspace_bytes, n, c)
                if nbytes < 0:
                    raise RuntimeError("average_precision: lgs_ap_workspace_bytes(%d, %d) failed" % (n, c))
                ws = _ws(nbytes, scores.device)
            engine.check(L.lgs_average_precision(_ptr(scores), n, c, _ptr(labels), int(ignore_index), 1 if from_logits else 0, _ptr(ap),
                                                 _dtype_code(scores), _ptr(ws), _stream()))
        return ap

    # ---- instance evaluation: lgs_inst_overlap
    INST_MAX_GT = 4096
    _INST_SCORE_MODE = {None: 0, "max": 1, "mean": 2}

    @staticmethod
    def inst_eval_fused():
        """tuning knob INST_EVAL_FUSED, read at call time (0 = the torch lines CPU tensors take, also on HIP tensors)"""
        return engine.tuning_get("INST_EVAL_FUSED") != 0

    def inst_overlap(self, member, offsets, n, gt_ids=None, valid_class_ids=None, g_cap=1024, scores=None, score_col=None, score_mode=None):
        """Proposals in CSR form (member [M] int32 point indices grouped by proposal, offsets [P + 1] int32) against the ground-truth
        ids [n] int64 of one scene -> (gt_id [g_cap] int64, gt_count [g_cap] int32, inter [P, g_cap] int32, prop_void [P] int32,
        conf [P] float32 or None, status [1] int32), all on the device, by the contract of lgs_inst_overlap in include/lgs_engine.h.
        score_mode "max" / "mean": conf[q] over scores[member of q, score_col[q]].  gt_ids None: conf alone.  No host sync."""
        _require_dev(member, "member")
        L = engine.lib()
        dev = member.device
        mode = self._INST_SCORE_MODE[score_mode]
        member = member.contiguous()
        offsets = offsets.contiguous()
        if member.dtype != torch.int32 or offsets.dtype != torch.int32:
            raise RuntimeError("inst_overlap: member and offsets must be int32")
        p, m = offsets.shape[0] - 1, member.shape[0]
        if gt_ids is not None:
            gt_ids = gt_ids.contiguous()
            valid_class_ids = valid_class_ids.contiguous()
            if gt_ids.dtype != torch.int64 or valid_class_ids.dtype != torch.int64 or gt_ids.shape[0] != n:
                raise RuntimeError("inst_overlap: gt_ids [n] and valid_class_ids must be int64")
        c = dt = 0
        if mode:
            scores = scores.detach().contiguous()
            score_col = score_col.contiguous()
            if scores.shape[0] != n or score_col.dtype != torch.int32 or score_col.shape[0] != p:
                raise RuntimeError("inst_overlap: scores must be [n, c] and score_col [P] int32")
            c, dt = scores.shape[1], _dtype_code(scores)
        with _dev(dev):
            gt_id = torch.empty(g_cap, dtype=torch.int64, device=dev)
            gt_count = torch.empty(g_cap, dtype=torch.int32, device=dev)
            inter = torch.empty((p, g_cap), dtype=torch.int32, device=dev)
            prop_void = torch.empty(p, dtype=torch.int32, device=dev)
            conf = torch.empty(p, dtype=torch.float32, device=dev) if mode else None
            status = torch.empty(1, dtype=torch.int32, device=dev)
            nbytes = memo(_QUERIES, ("inst_ws", n, m, p, g_cap), L.lgs_inst_overlap_workspace_bytes, n, m, p, g_cap)
            if nbytes < 0:
                raise RuntimeError("inst_overlap: lgs_inst_overlap_workspace_bytes(%d, %d, %d, %d) failed" % (n, m, p, g_cap))
            ws = _ws(nbytes, dev)
            engine.check(L.lgs_inst_overlap(_ptr(member), _ptr(offsets), _ptr(score_col) if mode else None, p, m, _ptr(gt_ids), n,
                                            _ptr(valid_class_ids) if gt_ids is not None else None,
                                            valid_class_ids.shape[0] if gt_ids is not None else 0, _ptr(scores) if mode else None, c, dt,
                                            mode, g_cap, _ptr(gt_id), _ptr(gt_count), _ptr(inter), _ptr(prop_void), _ptr(conf), _ptr(status),
                                            _ptr(ws), _stream()))
        return gt_id, gt_count, inter, prop_void, conf, status

    # ---- supervised point-contrastive loss: lgs_supcon_sample / lgs_supcon_forward / lgs_supcon_backward
    SUPCON_MAX_SAMPLES = 8
    _SUPCON_DISTANCE = {"cos": engine.LGS_SUPCON_COS, "l2": engine.LGS_SUPCON_L2}

    @staticmethod
    def supcon_enabled():
        """tuning knob SUPCON_FUSED, read at call time (0 = the torch gather path, also on HIP tensors)"""
        return engine.tuning_get("SUPCON_FUSED") != 0

    def supcon_sample(self, labels, n_labels, ignore_label, tables, p, k, seed):
        """-> (pos_idx [N, P], neg_idx [N, K]) int64, -1 = no sample (k_supcon_sample).  tables = (cum [L, L], order [N],
        seg_start [L], cls_count [L], elig_count [L]), device int64; seed: a host integer.  No host sync."""
        _require_dev(labels, "labels")
        L = engine.lib()
        labels = _int64(labels)
        cum, order, seg_start, cls_count, elig_count = (_int64(t) for t in tables)
        n = labels.shape[0]
        if tuple(cum.shape) != (n_labels, n_labels) or order.shape[0] != n or any(t.shape[0] != n_labels for t in (seg_start, cls_count, elig_count)):
            raise RuntimeError("supcon_sample: tables do not match %d rows and %d labels" % (n, n_labels))
        with _dev(labels.device):
            pos = torch.empty(n, p, dtype=torch.int64, device=labels.device)
            neg = torch.empty(n, k, dtype=torch.int64, device=labels.device)
            engine.check(L.lgs_supcon_sample(_ptr(labels), n, int(n_labels), int(ignore_label), _ptr(cum), _ptr(order), _ptr(seg_start),
                                             _ptr(cls_count), _ptr(elig_count), int(p), int(k), int(seed) & 0x7fffffffffffffff,
                                             _ptr(pos), _ptr(neg), _stream()))
        return pos, neg

    def supcon_forward(self, feats, labels, pos_idx, neg_idx, ignore_label, n_labels, distance):
        """one pass: -> (d_pos [N], d_neg [N], saved-for-backward tuple); sim [N, P + K] and inv_norm [N] are in the tuple"""
        _require_dev(feats, "features")
        L = engine.lib()
        feats = feats.contiguous()
        labels = _int64(labels)
        pos_idx, neg_idx = _int64(pos_idx), _int64(neg_idx)
        n, c = feats.shape
        p, k = pos_idx.shape[1], neg_idx.shape[1]
        if labels.shape[0] != n or pos_idx.shape[0] != n or neg_idx.shape[0] != n:
            raise RuntimeError("supcon_forward: labels / sample indices do not match %d rows" % n)
        dev = feats.device
        with _dev(dev):
            d_pos = torch.empty(n, dtype=torch.float32, device=dev)
            d_neg = torch.empty(n, dtype=torch.float32, device=dev)
            sim = torch.empty(n, p + k, dtype=torch.float32, device=dev)
            inv = torch.empty(n, dtype=torch.float32, device=dev)
            engine.check(L.lgs_supcon_forward(_ptr(feats), n, c, _ptr(labels), _ptr(pos_idx), p, _ptr(neg_idx), k, int(ignore_label),
                                              int(n_labels), self._SUPCON_DISTANCE[distance], _ptr(d_pos), _ptr(d_neg), _ptr(sim), _ptr(inv),
                                              _dtype_code(feats), _stream()))
        return d_pos, d_neg, (feats, labels, pos_idx, neg_idx, sim, inv)

    def supcon_backward(self, saved, g_dpos, g_dneg, ignore_label, n_labels, distance):
        """-> d loss / d features [N, C] in the features' dtype; g_dpos / g_dneg [N] or None"""
        L = engine.lib()
        feats, labels, pos_idx, neg_idx, sim, inv = saved
        n, c = feats.shape
        with _dev(feats.device):
            gf = torch.empty_like(feats)
            gp = _grad32(g_dpos)
            gn = _grad32(g_dneg)
            engine.check(L.lgs_supcon_backward(_ptr(feats), n, c, _ptr(labels), _ptr(pos_idx), pos_idx.shape[1], _ptr(neg_idx),
                                               neg_idx.shape[1], int(ignore_label), int(n_labels), self._SUPCON_DISTANCE[distance],
                                               _ptr(sim), _ptr(inv), _ptr(gp), _ptr(gn), _ptr(gf), _dtype_code(feats), _stream()))
        return gf

    def _one(self, device):
        """a device-resident 1.0f (the kernels take their scalar factors from device memory)"""
        cache = self.__dict__.setdefault("_one_cache", {})
        t = cache.get(device.index)
        if t is None:
            t = cache[device.index] = torch.ones((), dtype=torch.float32, device=device)
        return t
